"""GPU: rr_wpcr (kernels_wpcr.hip) against the sequential statement of Wpcr in tests/wpcr_model.py.  Four invariants are held on
every burst of every test here (check_burst):

  S  the magnitudes the decision was taken on (rr_debug_wpcr_spectrum) are within bound_spectrum of the float64 DFT of the burst's
     0/1 pulse vector
  B  whatever the input, `bin` is find_best_bin applied to the block's OWN f32 magnitudes, and ok = 0 exactly when that is None
  C  sps == fl32(bin) / fl32(n) bit for bit; phase0 within bound / |X[bin]| / 2 pi + 3 2^-24 of the float64 model, modulo 1
  G  exact: the symbols, nsyms and the phase tag are picks_exact run from the REPORTED phase0 and sps; the values are x[i] - mid
     bit for bit
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import rustradio_amd as rr
import wpcr_model as wm
from bits_model import G3RUH, HDLC_FLAG, Chain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T, CH, BT = 2048, 1024, 1024          # WPCR_T (samples of a tile), WPCR_CH (crossings of a chunk), WPCR_BT (bins of a tile): kernels.hpp


def test_tile_constants_mirror_the_kernel():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "kernels.hpp")).read()
    assert f"constexpr int WPCR_T = {T};" in src and f"constexpr int WPCR_BT = {BT};" in src and f"constexpr int WPCR_CH = {CH};" in src


def bits_of(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_burst(w, b, xb, mid, r, symsb, stats=None):
    """S, B, C and G for burst b of the latest call: xb its samples, mid its offset (None: 0), r its record, symsb the output
    buffer from its start on"""
    n, N = len(xb), max(len(xb) - 1, 0)
    m = F32(0.0) if mid is None else F32(mid)
    d = wm.pulses(xb, m) if n >= 2 else np.zeros(0)
    C = int(d.sum())
    X = np.fft.fft(d)[:N // 2] if N >= 2 else np.zeros(0, np.complex128)
    bound = wm.bound_spectrum(C)
    mag = w.spectrum(b)
    # S
    assert mag.dtype == np.float32 and len(mag) == N // 2
    err = np.abs(mag.astype(np.float64) - np.abs(X))
    assert np.all(err <= bound), (b, n, C, float(err.max()), bound)
    if stats is not None and C and len(err):
        stats["S"] = max(stats.get("S", 0.0), float(err.max()) / bound)
    # B
    want = wm.find_best_bin(mag) if n >= 4 else None
    assert bool(r["ok"]) == (want is not None), (b, n, want, r)
    if want is None:
        assert int(r["nsyms"]) == 0 and int(r["bin"]) == 0
        return None
    assert int(r["bin"]) == want, (b, n, want, r)
    # C
    assert bits_of(r["sps"]) == bits_of(F32(want) / F32(n))
    p64 = 0.5 + np.angle(X[want]) / (2.0 * np.pi)
    dp = abs(float(r["phase0"]) - p64) % 1.0
    with np.errstate(divide="ignore"):       # (an exact zero the block's own rounding noise made a line of: any phase)
        tol = bound / abs(X[want]) / (2.0 * np.pi) + 3 * 2.0 ** -24
    assert min(dp, 1.0 - dp) <= tol, (b, n, float(r["phase0"]), p64, tol)
    assert F32(0.5) < r["phase0"] <= F32(1.5)
    if stats is not None:
        stats["C"] = max(stats.get("C", 0.0), min(dp, 1.0 - dp) / tol)
    # G
    taken, nsyms, end = wm.picks_exact(r["phase0"], r["sps"], n)
    assert int(r["nsyms"]) == nsyms and bits_of(r["phase"]) == bits_of(end), (b, n, r, nsyms, end)
    got = symsb[:nsyms]
    with np.errstate(invalid="ignore"):
        ref = xb[taken] if mid is None else (xb[taken] - m).astype(F32)
    if mid is None:
        assert np.array_equal(bits_of(got), bits_of(ref)), (b, n)
    else:
        assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(ref)), (b, n)
    return want


def run_and_check(w, x, starts, lens, mids=None, stats=None):
    """one host-form call over the batch, every burst held to S, B, C, G -> (records, syms)"""
    syms = w.process_buffer(x, starts, lens, mids)
    res = w.results()
    assert len(res) == len(starts) and len(syms) == len(x)
    for b, (s, n) in enumerate(zip(starts, lens)):
        check_burst(w, b, x[s:s + n], None if mids is None else mids[b], res[b], syms[s:], stats)
    return res, syms


def noisy_nrz(n, seed, sps=6.37):
    """n samples of random NRZ at a non-integer number of samples per symbol"""
    rng = np.random.default_rng(seed)
    x = wm.upsample_nrz(rng.choice([-1.0, 1.0], int(n / sps) + 3), sps, rng)
    assert len(x) >= n
    return x[:n]


# ---- 1. tiny bursts, exhaustively ---------------------------------------------------------------------------------------------------
def test_every_sign_pattern_of_every_length_up_to_12():
    """n = 0 .. 12, every 0/1 pattern: 8191 bursts touching each other in one batch — n < 4, odd and even N, N / 2 of 2, 3 and 4
    and beyond, one crossing, all-alternating (C = N)"""
    rng = np.random.default_rng(5)
    parts, lens = [], []
    for n in range(13):
        pat = (np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1
        parts.append((np.where(pat == 1, 1.0, -1.0) * rng.uniform(0.25, 2.0, pat.shape)).astype(F32).ravel())
        lens += [n] * 2 ** n
    x = np.concatenate(parts)
    lens = np.array(lens)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert len(lens) == 8191
    w = rr.Wpcr()
    stats = {}
    res, _ = run_and_check(w, x, starts, lens, stats=stats)
    assert not res["ok"][lens < 9].any()             # N / 2 <= 3 up to n = 8
    assert res["ok"][lens >= 9].any() and not res["ok"][lens >= 9].all()
    print(f"valid: {int(res['ok'].sum())} of 8191; allowance used: {stats}")


# ---- 2. builder bursts against the reference's rule ------------------------------------------------------------------------------------
def test_builder_bursts_choose_the_bin_the_float64_model_chooses():
    """the AX.25-like bursts of the model's builder, odd starts and gaps between them, with a sample rate: wherever the margin of
    find_best_bin's decisions exceeds 4 bound_spectrum the bin is the float64 model's; at most 5 % may fall under that margin"""
    rng = np.random.default_rng(11)
    bursts = [wm.nrz_burst(s) for s in wm.GPU_SEEDS]
    gaps = [2 * int(g) + 1 for g in rng.integers(0, 40, len(bursts))]
    starts, at = [], 1
    for bst, g in zip(bursts, gaps):
        starts.append(at)
        at += len(bst) + g
    x = rng.normal(0.0, 1.0, at).astype(F32)
    for s, bst in zip(starts, bursts):
        x[s:s + len(bst)] = bst
    lens = [len(bst) for bst in bursts]
    w = rr.Wpcr(samp_rate=50000.0)
    stats = {}
    res, syms = run_and_check(w, x, starts, lens, stats=stats)
    left_out = 0
    for b, bst in enumerate(bursts):
        X = wm.spectrum64(bst)
        C = int(wm.pulses(bst).sum())
        want, gap = wm.best_bin_margin(np.abs(X))
        if gap <= 4 * wm.bound_spectrum(C):
            left_out += 1
            continue
        assert res[b]["ok"] and int(res[b]["bin"]) == want, (b, want, res[b])
        assert bits_of(res[b]["frequency"]) == bits_of(res[b]["sps"] * F32(50000.0))
    assert left_out <= 0.05 * len(bursts)
    print(f"{len(bursts)} bursts, {left_out} under the margin; allowance used: {stats}")


# ---- 3. shapes --------------------------------------------------------------------------------------------------------------------
def test_lengths_around_every_tile_size():
    """n - 1 (the pulses) and n (the samples) one below, at and one above the sample tile; N / 2 one below, at and one above the
    bin tile; all-alternating bursts with one crossing less than, exactly and one more than a crossing chunk in their tile, and
    with every chunk of two tiles full; 3 x the largest tile + 1; odd starts; bursts that touch; dropped bursts in between"""
    lens = [T - 1, T, T + 1, T + 2, 2 * BT - 1, 2 * BT, 2 * BT + 1, 2 * BT + 2, 2 * BT + 3, 2 * BT + 4, 3, 3 * T + 1, 0, 2 * T, 2 * T + 1, 1, 7,
            CH, CH + 1, CH + 2]
    gaps = [0, 1, 0, 3, 0, 0, 5, 0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0]
    starts, at = [], 3
    for n, g in zip(lens, gaps):
        starts.append(at)
        at += n + g
    x = np.zeros(at + 5, F32)
    for j, (s, n) in enumerate(zip(starts, lens)):
        if n == 2 * T or j >= 17:
            x[s:s + n] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)      # all-alternating: C = N
        elif n:
            x[s:s + n] = noisy_nrz(n, 100 + j)
    w = rr.Wpcr()
    stats = {}
    res, _ = run_and_check(w, x, starts, lens, stats=stats)
    ok = res["ok"].astype(bool)
    assert ok[[0, 1, 2, 3, 11, 14]].all() and not ok[[10, 12, 15, 16]].any()
    print(f"allowance used: {stats}")


@pytest.mark.parametrize("nb", [1, 2, 257])
def test_number_of_bursts(nb):
    rng = np.random.default_rng(nb)
    lens = [int(v) for v in rng.integers(0, 160, nb)]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int) + 1
    x = np.zeros(sum(lens) + 2, F32)
    for j, (s, n) in enumerate(zip(starts, lens)):
        if n:
            x[s:s + n] = noisy_nrz(n, 300 + j, sps=4.6)
    res, _ = run_and_check(rr.Wpcr(), x, starts, lens)
    if nb == 257:
        assert res["ok"].any() and not res["ok"].all()


def test_pure_noise_and_a_pure_tone():
    """the invariants do not depend on there being a clock to find"""
    rng = np.random.default_rng(21)
    noise = rng.normal(0.0, 1.0, 3001).astype(F32)
    tone = np.sin(2 * np.pi * np.arange(2500) / 7.3 + 0.4).astype(F32)
    x = np.concatenate([noise, tone])
    run_and_check(rr.Wpcr(), x, [0, 3001], [3001, 2500])


# ---- 4. mid ---------------------------------------------------------------------------------------------------------------------
def test_mid_equals_shifting_the_burst_on_the_host():
    bursts = [noisy_nrz(n, 400 + j) for j, n in enumerate((700, 1501, 2300))]
    mids = np.array([0.37, -1.25, 0.001], F32)
    lens = [len(b) for b in bursts]
    starts = [0, 700, 700 + 1501]
    raw = np.concatenate([b + m for b, m in zip(bursts, mids)]).astype(F32)
    shifted = np.concatenate([(raw[s:s + n] - m).astype(F32) for s, n, m in zip(starts, lens, mids)])
    w = rr.Wpcr()
    res_a, syms_a = run_and_check(w, raw, starts, lens, mids)
    res_b, syms_b = run_and_check(w, shifted, starts, lens)
    assert res_a["ok"].all() and res_a.tobytes() == res_b.tobytes()
    for s, r in zip(starts, res_a):
        k = int(r["nsyms"])
        assert np.array_equal(bits_of(syms_a[s:s + k]), bits_of(syms_b[s:s + k]))


def test_nan_mid_drops_the_burst_and_nonfinite_samples_pass_through():
    a, b, c = noisy_nrz(900, 500), noisy_nrz(1200, 501), noisy_nrz(800, 502)
    b = b.copy()
    b[100:110] = np.nan                      # slices as 0
    b[400] = np.inf                          # ... 1
    b[401:405] = -np.inf                     # ... 0
    b[700:703] = np.array([np.nan, np.inf, -np.inf], F32)
    x = np.concatenate([a, b, c])
    starts, lens = [0, 900, 2100], [900, 1200, 800]
    w = rr.Wpcr()
    res, syms = run_and_check(w, x, starts, lens)
    assert res["ok"].all()
    k = int(res[1]["nsyms"])
    assert not np.isfinite(syms[900:900 + k]).all()          # some non-finite samples were picked, and copied bit for bit (G)
    res, _ = run_and_check(w, x, starts, lens, np.array([0.0, np.nan, 0.1], F32))
    assert res["ok"].tolist() == [1, 0, 1]
    res, _ = run_and_check(w, x, starts, lens, np.array([np.inf, 0.0, -np.inf], F32))
    assert res["ok"].tolist() == [0, 1, 0]


# ---- 5. host and device forms -------------------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree_and_a_smaller_batch_leaves_nothing_behind():
    lens = [1000, 0, 2500, 3, 1700]
    starts = [5, 1005, 1006, 3506, 3511]
    x = np.zeros(5300, F32)
    for j, (s, n) in enumerate(zip(starts, lens)):
        if n:
            x[s:s + n] = noisy_nrz(n, 600 + j)
    mids = np.array([0.0, 0.0, 0.05, 0.0, -0.02], F32)
    w = rr.Wpcr(samp_rate=48000.0)
    res_h, syms_h = run_and_check(w, x, starts, lens, mids)
    d_x = torch.from_numpy(x).cuda()
    d_s = torch.full((len(x),), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    l0 = int(rr.lib().rr_debug_kernel_launches())
    w.process_dev(d_x.data_ptr(), len(x), starts, lens, mids, d_s.data_ptr())
    assert int(rr.lib().rr_debug_kernel_launches()) - l0 == 4
    res_d = w.results()
    syms_d = d_s.cpu().numpy()
    assert res_d.tobytes() == res_h.tobytes()
    untouched = np.ones(len(x), bool)
    for s, r in zip(starts, res_d):
        k = int(r["nsyms"])
        assert np.array_equal(bits_of(syms_d[s:s + k]), bits_of(syms_h[s:s + k]))
        untouched[s:s + k] = False
    assert np.all(syms_d[untouched] == -7.0)                  # the rest of d_syms is left alone
    # a smaller batch on the same handle: its own records only
    w.process_dev(d_x.data_ptr(), len(x), starts[2:3], lens[2:3], None, d_s.data_ptr())
    res2 = w.results()
    assert len(res2) == 1 and res2[0]["ok"]
    with pytest.raises(RuntimeError, match="no such burst"):
        w.spectrum(1)
    check_burst(w, 0, x[starts[2]:starts[2] + lens[2]], None, res2[0], d_s.cpu().numpy()[starts[2]:])
    # an empty batch launches nothing and has no records
    l0 = int(rr.lib().rr_debug_kernel_launches())
    w.process_dev(d_x.data_ptr(), len(x), [], [], None, d_s.data_ptr())
    assert int(rr.lib().rr_debug_kernel_launches()) == l0 and len(w.results()) == 0
    assert w.process([]) == []


def test_process_returns_packets_and_none():
    w = rr.Wpcr(samp_rate=50000.0)
    good = wm.nrz_burst(wm.GPU_SEEDS[0])
    out = w.process([good, np.ones(50, F32), good[:3]])
    assert out[1] is None and out[2] is None
    syms, tags = out[0]
    r = w.results()[0]
    assert len(syms) == int(r["nsyms"]) and set(tags) == {"sps", "phase", "frequency"}
    assert set(rr.Wpcr().process([good])[0][1]) == {"sps", "phase"}
    with pytest.raises(RuntimeError, match="whole bursts"):
        w.work(good, len(good))


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    w = rr.Wpcr()
    n_total = rr.WPCR_MAX_LEN + 10
    d_x = torch.zeros(n_total, dtype=torch.float32, device="cuda")
    d_s = torch.zeros(n_total, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    l0 = int(rr.lib().rr_debug_kernel_launches())
    for starts, lens, msg in (([0, 99], [100, 50], "bursts overlap"), ([200, 100], [10, 10], "bursts overlap"),
                              ([0, n_total - 5], [10, 6], "burst outside the buffer"), ([n_total + 1], [0], "burst outside the buffer"),
                              ([0], [rr.WPCR_MAX_LEN + 1], "burst longer than 512000 samples")):
        with pytest.raises(RuntimeError, match=msg):
            w.process_dev(d_x.data_ptr(), n_total, starts, lens, None, d_s.data_ptr())
        with pytest.raises(RuntimeError, match=msg):
            w.process_buffer(np.zeros(n_total, F32), starts, lens)
    assert int(rr.lib().rr_debug_kernel_launches()) == l0
    # touching is not overlapping, and a burst may end exactly at the buffer's end
    w.process_dev(d_x.data_ptr(), n_total, [0, 100, n_total - 50], [100, 30, 50], None, d_s.data_ptr())
    assert len(w.results()) == 3 and not w.results()["ok"].any()
    other = rr.BinarySlicer()
    total = C.c_size_t(0)
    assert rr.lib().rr_wpcr_results(other._h, None, 0, C.byref(total)) == rr.ERR and "not a wpcr handle" in rr.last_error()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------
def test_end_to_end_g3ruh_frame_through_the_bit_decoder():
    """a G3RUH-scrambled, NRZI-coded payload between HDLC flags at 5.2083 samples per symbol: rr.Wpcr -> rr.BitDecoder gives the
    bits and flag tags of the sequential model chain, which itself recovers the planted bits without error"""
    x, tx = wm.g3ruh_burst(1)
    m_syms, m_tags, m_bin, m_p0 = wm.process_one(x, samp_rate=50000.0)
    m_bits, m_pos, m_diffs = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG).run(m_syms)
    assert wm.planted_offset(m_bits, tx) is not None                  # the CPU side: the model chain decodes what was sent
    w = rr.Wpcr(samp_rate=50000.0)
    (syms, tags), = w.process([x])
    check_burst(w, 0, x, None, w.results()[0], syms)
    assert int(w.results()[0]["bin"]) == m_bin and bits_of(tags["sps"]) == bits_of(m_tags["sps"])
    dec = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    st, c, p, need, bits = dec.work(syms, len(syms))
    pos, diffs = dec.tags()
    assert np.array_equal(bits, m_bits)
    assert np.array_equal(pos, m_pos) and np.array_equal(diffs, m_diffs) and len(pos) >= 3


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_wpcr(tmp_path):
    rate = 9600.0 * 5.2083
    bursts = [wm.g3ruh_burst(1)[0], noisy_nrz(1500, 700), np.ones(64, F32), noisy_nrz(2300, 701) + F32(0.4), noisy_nrz(3, 702)]
    mids = np.array([0.0, 0.0, 0.0, 0.4, 0.0], F32)
    w = rr.Wpcr(samp_rate=rate)
    out = w.process(bursts, mids)
    res = w.results()
    assert [o is not None for o in out] == [True, True, False, True, False]
    vec = tmp_path / "vectors.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<fQ", rate, len(bursts)))
        for bst, m, o, r in zip(bursts, mids, out, res):
            syms = o[0] if o is not None else np.zeros(0, F32)
            f.write(struct.pack("<Q", len(bst))); f.write(np.ascontiguousarray(bst, "<f4").tobytes())
            f.write(struct.pack("<fBQ", float(m), int(r["ok"]), len(syms))); f.write(syms.astype("<f4").tobytes())
            f.write(struct.pack("<fff", float(r["sps"]), float(r["phase"]), float(r["frequency"])))
    exe = os.path.join(ROOT, "tests", "cpp", "test_wpcr_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_wpcr_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
