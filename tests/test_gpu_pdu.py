"""GPU: rr_stream_to_pdu (kernels_pdu.hip) against the sequential models of tests/pdu_model.py, its glue to rr_wpcr
(rr_wpcr_process_pdus, rr_wpcr_pack_dev) and the receive chain of examples/ax25-9600-wpcr.rs end to end.

Every comparison of PDUs is bit for bit and per push: which push reports a PDU, its absolute position, its samples, and that
the records are ascending, disjoint and inside the arena."""
import os

import numpy as np
import pytest
import torch

import hdlc_model as hm
import pdu_model as pm
import rustradio_amd as rr
import wpcr_model as wm
from bits_model import G3RUH, nrzi_encode, scramble

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T = 2048                    # PDU_T (samples of a tile): kernels.hpp


def test_tile_constant_mirrors_the_kernel():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "kernels.hpp")).read()
    assert f"constexpr int PDU_T = {T};" in src


def bits_of(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def labelled(n, seed=0):
    """n distinct, finite samples: a PDU with the wrong samples cannot pass for the right one"""
    return (np.arange(n, dtype=np.float64) * 0.25 - 100.0 + np.random.default_rng(seed).uniform(0, 0.2, n)).astype(F32)


def push_all(b, x, trig, splits):
    """the stream through b, cut at `splits` -> per push [(stream_pos, samples)]; the records' geometry is checked on the way"""
    cuts = [0] + sorted(splits) + [len(x)]
    per = []
    for a, c in zip(cuts[:-1], cuts[1:]):
        rec = b.push(x[a:c], trig[a:c])
        p, n_total = b.arena_dev()
        assert (n_total == 0 and p is None and len(rec) == 0) if c == a else (n_total > 0 and p)
        end = 0
        for r in rec:
            assert int(r["start"]) >= end and int(r["start"]) + int(r["len"]) <= n_total, (r, n_total)
            end = int(r["start"]) + int(r["len"])
        per.append([(int(r["stream_pos"]), b.pdu(i, rec)) for i, r in enumerate(rec)])
    return per


def check_stream(x, trig, thr, max_size, tail, splits=(), flags=0, b=None):
    """-> the block, after its PDUs have been held against the sequential model push by push"""
    want = pm.stream_to_pdu_seq(x, trig, thr, max_size, tail, splits)
    b = rr.StreamToPdu(thr, max_size, tail, flags) if b is None else b
    got = push_all(b, x, trig, splits)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert [f for f, _ in g] == [f for f, _ in w], (k, [(f, len(p)) for f, p in g], [(f, len(p)) for f, p in w])
        for (f, gp), (_, wp) in zip(g, w):
            assert np.array_equal(bits_of(gp), bits_of(np.array(wp, F32))), (k, f)
    return b, want


def trigger_of(n, bursts):
    t = np.zeros(n, F32)
    for r, length in bursts:
        t[r:r + length] = 1.0
    return t


# ---- 1. windows and bursts around the tile ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [T - 1, T, T + 1, 2 * T + 1])
def test_windows_and_bursts_around_the_tile(window):
    """three pushes of `window` samples; bursts of 1, 2, 3, T - 1 and T + 1 samples, some of them across a push boundary"""
    n = 3 * window
    lens = [1, 2, 3, T - 1, 1, T + 1, 3, 2]
    gap = (n - sum(lens)) // (len(lens) + 1)
    assert gap >= 4
    at, bursts = gap, []
    for length in lens:
        bursts.append((at, length))
        at += length + gap
    b, want = check_stream(labelled(n), trigger_of(n, bursts), 0.5, T + 8, 2, [window, 2 * window])
    assert sum(len(w) for w in want) == len(lens)


# ---- 2. a burst cut at every position ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1, 50])
def test_a_burst_cut_at_every_split_position(tail):
    """ONE handle, one stream: segment s of 120 samples holds a burst at [10, 20) and is cut s samples in — before the burst, in
    it, on its falling edge, at every position of its tail, behind it"""
    seg, parts, splits = 120, [], []
    for s in range(1, 100):
        parts.append(trigger_of(seg, [(10, 10)]))
        splits += [seg * (s - 1) + s, seg * s]
    trig = np.concatenate(parts)
    b, want = check_stream(labelled(len(trig)), trig, 0.5, 64, tail, splits[:-1])
    assert sum(len(w) for w in want) == 99
    assert any(len(w) == 0 for w in want)


def test_a_burst_across_three_pushes_and_a_tail_longer_than_a_push():
    n = 400
    trig = trigger_of(n, [(50, 200)])
    check_stream(labelled(n), trig, 0.5, 300, 3, [100, 200])
    check_stream(labelled(n), trig, 0.5, 300, 60, [100, 200, 251, 252, 260, 300])      # the tail spans four pushes
    check_stream(labelled(n), trig, 0.5, 300, 3, list(range(1, n)))                     # one sample per push


def test_max_size_met_and_one_more():
    n = 200
    for L, tail, max_size, npdus in [(30, 10, 40, 1), (30, 10, 39, 0), (40, 0, 40, 1), (41, 0, 40, 0), (1, 0, 1, 1), (1, 1, 1, 0),
                                     (5, 0, 0, 0)]:
        for splits in ([], [60], [75], [82]):
            b, want = check_stream(labelled(n), trigger_of(n, [(50, L), (150, 3)]), 0.5, max_size, tail, splits)
            assert sum(len(w) for w in want) == npdus + (1 if 3 + tail <= max_size else 0)


def test_rising_edges_inside_a_tail_and_behind_a_burst_that_was_too_long():
    n = 300
    # a second burst begins inside the first one's tail: ignored WITH its falling edge, even though that lies behind the tail
    check_stream(labelled(n), trigger_of(n, [(20, 10), (33, 30), (100, 5)]), 0.5, 64, 8, [35])
    check_stream(labelled(n), trigger_of(n, [(20, 10), (33, 30), (100, 5)]), 0.5, 64, 8, [31, 36, 50])
    # too long: free = r + max_size + 1; a burst that begins before that is ignored, one that begins at it is taken
    check_stream(labelled(n), trigger_of(n, [(20, 50), (80, 4)]), 0.5, 30, 0)
    check_stream(labelled(n), trigger_of(n, [(20, 28), (50, 4), (60, 4)]), 0.5, 30, 5, [40])
    check_stream(labelled(n), trigger_of(n, [(20, 28), (51, 4), (60, 4)]), 0.5, 30, 5, [49, 51])


@pytest.mark.parametrize("max_size,tail", [(4, 0), (3, 1), (6, 5), (40, 37)])
def test_a_trigger_that_toggles_every_sample(max_size, tail):
    """2 T + 1 samples, an edge at every one: the densest edge list and, with a long tail, the longest chains of ignored edges"""
    n = 2 * T + 1
    trig = (np.arange(n) % 2 == 0).astype(F32)
    b, want = check_stream(labelled(n), trig, 0.5, max_size, tail)
    pos, val = b.edges()
    assert np.array_equal(pos, np.arange(n)) and np.array_equal(val, np.arange(n) % 2 == 0)
    assert sum(len(w) for w in want) >= n // (2 * (tail + 2))
    check_stream(labelled(n), trig, 0.5, max_size, tail, [T - 1, T + 1])


def test_a_burst_at_sample_0_nan_trigger_nan_threshold_and_empty_pushes():
    n = 64
    check_stream(labelled(n), trigger_of(n, [(0, 5), (20, 5)]), 0.5, 16, 1)
    t = trigger_of(n, [(10, 20)])
    t[15] = np.nan                                                   # not above: the burst falls there and rises again
    b, want = check_stream(labelled(n), t, 0.5, 32, 0)
    assert [len(p) for _, p in want[0]] == [5, 14]
    b, want = check_stream(labelled(n), t, np.nan, 32, 0)
    assert want == [[]] and len(b.edges()[0]) == 0
    # n == 0 between two halves of a burst: nothing reported, nothing forgotten
    b, want = check_stream(labelled(n), trigger_of(n, [(10, 20)]), 0.5, 32, 2, [0, 15, 15, 15, n])
    assert [len(w) for w in want] == [0, 0, 0, 0, 1, 0]
    with pytest.raises(RuntimeError, match="forms PDUs"):
        b.work(np.zeros(4, F32), 4)                                  # a PDU-forming block has no stream protocol


def test_random_streams_and_splits():
    rng = np.random.default_rng(21)
    for it in range(12):
        n = int(rng.integers(1, 3 * T))
        run = int(rng.choice([1, 3, 40]))
        trig = np.repeat(rng.random(n // run + 1) < 0.5, run)[:n].astype(F32)
        splits = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 5))))
        check_stream(labelled(n, it), trig, 0.5, int(rng.integers(0, 3 * run + 4)), int(rng.integers(0, run + 3)), splits)


# ---- 3. the edges are the burst detector's -------------------------------------------------------------------------------------------
def test_edges_equal_the_burst_detectors():
    rng = np.random.default_rng(3)
    n = 3 * T + 17
    amp = np.repeat(rng.random(n // 97 + 1) < 0.4, 97)[:n] * 1.0
    x = (amp * np.exp(2j * np.pi * rng.random(n)) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    det, b = rr.BurstDetector(0.05, 0.3), rr.StreamToPdu(0.3, 500, 10)
    for a, c in [(0, T + 5), (T + 5, T + 6), (T + 6, n)]:
        st, cons, prod, need, env = det.work(x[a:c], c - a)
        assert prod == c - a
        b.push(np.zeros(c - a, F32), env)
        (p0, v0), (p1, v1) = det.edges(), b.edges()
        assert len(p0) > 0 or c - a == 1
        assert np.array_equal(p0, p1) and np.array_equal(v0, v1)


# ---- 4. Midpointer --------------------------------------------------------------------------------------------------------------------
def midpoint_records(bursts, max_size=None, gap=3):
    """every burst as one PDU of ONE push (trigger high over it, tail 0) -> records, in order"""
    max_size = max(len(v) for v in bursts) if max_size is None else max_size
    xs, ts = [np.zeros(gap, F32)], [np.zeros(gap, F32)]
    for v in bursts:
        xs += [np.ascontiguousarray(v, F32), np.zeros(gap, F32)]
        ts += [np.ones(len(v), F32), np.zeros(gap, F32)]
    b = rr.StreamToPdu(0.5, max_size, 0, rr.PDU_MIDPOINT)
    rec = b.push(np.concatenate(xs), np.concatenate(ts))
    assert [int(r["len"]) for r in rec] == [len(v) for v in bursts]
    return rec, b


def check_ranks(b, i, m):
    """low and high of PDU i (rr_debug_pdu_ranks) are the model's, bit for bit"""
    low, high = b.ranks(i)
    want = (m["low"], m["high"]) if m["ok"] else (F32(0), F32(0))
    assert bits_of(low) == bits_of(want[0]) and bits_of(high) == bits_of(want[1]), (i, low, high, want)


def check_exact(rec, bursts, b=None):
    for i, (r, v) in enumerate(zip(rec, bursts)):
        m = pm.midpointer_block(v)
        if b is not None:
            check_ranks(b, i, m)
        assert int(r["ok"]) == m["ok"] and int(r["nlow"]) == m["nlow"], (r, m)
        assert bits_of(r["mean"]) == bits_of(m["mean"]) or (np.isnan(r["mean"]) and np.isnan(m["mean"])), (r, m)
        assert bits_of(r["mid"]) == bits_of(m["mid"]), (r, m)


def test_midpointer_exact_arithmetic():
    """multiples of 2^-10 below 2^13: the f64 sum is exact in any order, so the whole record equals the model bit for bit"""
    rng = np.random.default_rng(31)
    bursts = [(rng.integers(-2 ** 23 + 1, 2 ** 23, n) * 2.0 ** -10).astype(F32) for n in (2, 3, 5, 64, 1023, 1024, 1025, 4099)]
    bursts.append((np.sign(rng.standard_normal(3000)) * 512 + rng.integers(-40, 40, 3000) * 2.0 ** -10 + 100).astype(F32))   # two levels
    rec, b = midpoint_records(bursts)
    assert all(int(r["ok"]) == 1 for r in rec)
    check_exact(rec, bursts, b)


def ulp_apart(a, b):
    ka, kb = pm.total_key(np.array([a], F32)).astype(np.int64)[0], pm.total_key(np.array([b], F32)).astype(np.int64)[0]
    return abs(int(ka) - int(kb))


def test_midpointer_arbitrary_floats():
    """mean within 1 ulp of fl32(fsum / len); nlow, low, high and mid exactly the model's from the REPORTED mean"""
    rng = np.random.default_rng(32)
    bursts = [pm.noisy_nrz_burst(rng, n, 5.2083, rng.uniform(-1, 1), 0.2) for n in (7, 500, 2049, 10000)]
    bursts += [rng.standard_normal(777).astype(F32) * F32(1e-20), (rng.standard_normal(3001) * 1e6 + 3e6).astype(F32),
               rng.standard_cauchy(1500).astype(F32)]
    rec, b = midpoint_records(bursts)
    for i, (r, v) in enumerate(zip(rec, bursts)):
        assert ulp_apart(r["mean"], pm.mean_exact(v)) <= 1, (r, pm.mean_exact(v))
        m = pm.midpointer_block(v, mean=r["mean"])
        assert int(r["ok"]) == m["ok"] == 1 and int(r["nlow"]) == m["nlow"] and bits_of(r["mid"]) == bits_of(m["mid"]), (r, m)
        check_ranks(b, i, m)


def test_midpointer_pushes_nothing():
    rng = np.random.default_rng(33)
    good = pm.noisy_nrz_burst(rng, 300, 6.0, 0.5, 0.1)
    with_nan = good.copy(); with_nan[17] = np.nan
    both_inf = good.copy(); both_inf[3], both_inf[250] = np.inf, -np.inf
    bursts = [good, with_nan, both_inf, np.full(100, 2.5, F32), np.full(65, np.inf, F32), good[::-1].copy()]
    rec, b = midpoint_records(bursts)
    assert [int(r["ok"]) for r in rec] == [1, 0, 0, 0, 0, 1]
    assert all(b.ranks(i) == (0, 0) for i in range(1, 5))
    with pytest.raises(RuntimeError, match="no such PDU"):
        b.ranks(6)
    assert np.isnan(rec[1]["mean"]) and np.isnan(rec[2]["mean"]) and int(rec[1]["nlow"]) == 300
    assert rec[3]["mean"] == F32(2.5) and int(rec[3]["nlow"]) == 100
    assert all(bits_of(r["mid"]) == 0 for r in rec[1:5])
    for k in (0, 5):
        m = pm.midpointer_block(bursts[k], mean=rec[k]["mean"])
        assert ulp_apart(rec[k]["mean"], pm.mean_exact(bursts[k])) <= 1 and int(rec[k]["nlow"]) == m["nlow"]
        assert bits_of(rec[k]["mid"]) == bits_of(m["mid"])
    # one infinity alone leaves an infinite mean: no sample is above it
    one_inf = good.copy(); one_inf[5] = np.inf
    rec, _ = midpoint_records([one_inf])
    m = pm.midpointer_block(one_inf)
    assert int(rec[0]["ok"]) == m["ok"] and int(rec[0]["nlow"]) == m["nlow"] and bits_of(rec[0]["mid"]) == bits_of(m["mid"])


def test_midpointer_signed_zeros_pick_by_total_order():
    # mean +0: both zeros are on the low side, and the rank decides which of them is `low`
    v = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1.0, -1.0, 0.0], F32)
    for burst in (v, v[::-1].copy(), np.array([-0.0, 0.0, -0.0, 2.0, -2.0], F32), np.array([0.0, -0.0, 4.0, -4.0], F32)):
        rec, b = midpoint_records([burst])
        m = pm.midpointer_block(burst)
        assert m["ok"] == 1 and int(rec[0]["ok"]) == 1 and int(rec[0]["nlow"]) == m["nlow"]
        check_ranks(b, 0, m)                                         # (-0.0 and +0.0 are told apart: the bits are compared)
        assert bits_of(rec[0]["mean"]) == bits_of(m["mean"]) and bits_of(rec[0]["mid"]) == bits_of(m["mid"]), (rec[0], m)
    low = pm.midpointer_block(np.array([-0.0, 0.0, -0.0, 2.0, -2.0], F32))["low"]
    assert low == 0 and np.signbit(low)


def test_midpointer_64_bursts_and_one_of_max_size():
    rng = np.random.default_rng(34)
    max_size = 40000
    grid = lambda n: (np.sign(rng.standard_normal(n)) * 300 + rng.integers(-2000, 2000, n) * 2.0 ** -10 + 7).astype(F32)
    bursts = [grid(int(rng.integers(200, 400))) for _ in range(40)] + [grid(max_size)] + [grid(int(rng.integers(2, 9))) for _ in range(24)]
    rec, b = midpoint_records(bursts, max_size)
    assert len(rec) == 65
    check_exact(rec, bursts, b)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
def fm_stream(seed=5, sps=5.2083, kf=0.35, offset=0.25):
    """two G3RUH bursts (HDLC frames, NRZI, scrambled, NRZ at a non-integer sps, off centre by `offset`) as a Complex FM
    baseband with silence between them -> (samples, payloads)"""
    rng = np.random.default_rng(seed)
    payloads = [bytes(rng.integers(0, 256, 40).tolist()), bytes(rng.integers(0, 256, 55).tolist())]
    freq, amp = [], []
    for gap, p in zip([700, 900, 600], payloads + [None]):
        freq.append(np.zeros(gap)); amp.append(np.zeros(gap))
        if p is not None:
            line = scramble(nrzi_encode(hm.frame_bits(p, flags_before=8, flags_after=4)) + [0] * 17)
            nrz = wm.upsample_nrz(2.0 * np.array(line, np.float64) - 1.0, sps, rng, noise=0.0).astype(np.float64)
            freq.append(kf * (nrz + offset)); amp.append(np.ones(len(nrz)))
    ph = np.cumsum(np.concatenate(freq))
    x = np.concatenate(amp) * np.exp(1j * ph) + 0.02 * (rng.standard_normal(len(ph)) + 1j * rng.standard_normal(len(ph)))
    return x.astype(np.complex64), payloads


def test_end_to_end_two_g3ruh_bursts_one_across_a_push():
    """rr_burst_detector + rr_quaddemod -> rr_stream_to_pdu -> rr_wpcr_process_pdus -> rr_wpcr_pack_dev -> rr_bit_decoder on
    device buffers; the host model of HdlcDeframer recovers both frames, and rr_hdlc_deframer, fed the same device buffer, what the
    model recovers: frames, positions and counters"""
    kf, thr = 0.35, 0.3
    x, payloads = fm_stream(kf=kf)
    n = len(x) - 1
    dx = torch.from_numpy(x.view(F32).copy()).cuda()
    env = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    data = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    det, dem = rr.BurstDetector(0.1, thr), rr.QuadratureDemod(1.0 / kf)
    assert det.work_dev(dx.data_ptr(), n + 1, env.data_ptr(), n + 1)[2] == n + 1
    assert dem.work_dev(dx.data_ptr(), n + 1, data.data_ptr(), n)[2] == n
    det.sync(); dem.sync()
    cut = 4800                                                       # inside the second burst
    pdus = rr.StreamToPdu(thr, 6000, 20, rr.PDU_MIDPOINT)
    w, dec = rr.Wpcr(samp_rate=50000.0), rr.BitDecoder(nrzi=True, descrambler=G3RUH)
    deframer, frames, seen = hm.HdlcModel(10, 200), [], []
    dev_deframer = rr.HdlcDeframer(10, 200)
    for a, c in [(0, cut), (cut, n)]:
        pdus.push_dev(data.data_ptr() + 4 * a, env.data_ptr() + 4 * a, c - a)
        rec = pdus.records()
        seen.append([(int(r["stream_pos"]), int(r["len"]), int(r["ok"])) for r in rec])
        p, n_total = pdus.arena_dev()
        syms = torch.zeros(n_total, dtype=torch.float32, device="cuda")
        w.process_pdus(pdus, syms.data_ptr())
        res = w.results()
        assert len(res) == sum(int(r["ok"]) for r in rec)
        cap = int(sum(int(r["nsyms"]) for r in res))
        packed = torch.zeros(max(cap, 1), dtype=torch.float32, device="cuda")
        produced, pst, pln = w.pack(syms.data_ptr(), packed.data_ptr(), cap)
        assert produced == cap and list(pln) == [int(r["nsyms"]) for r in res if r["ok"] and r["nsyms"]]
        assert list(pst) == list(np.cumsum([0] + list(pln))[:-1])
        if cap:
            with pytest.raises(RuntimeError, match="output shorter than the packed symbols"):
                w.pack(syms.data_ptr(), packed.data_ptr(), cap - 1)
            # the packed stream is the bursts' symbols minus their mids, back to back
            hs, at = syms.cpu().numpy(), 0
            ok = [r for r in rec if r["ok"]]
            for r, q in zip(ok, res):
                k = int(q["nsyms"])
                assert np.array_equal(bits_of(packed.cpu().numpy()[at:at + k]), bits_of(hs[int(r["start"]):int(r["start"]) + k]))
                at += k
            bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            assert dec.work_dev(packed.data_ptr(), cap, bits.data_ptr(), cap)[2] == cap
            dec.sync()
            ended = deframer.run(bits.cpu().numpy())
            frames += ended
            dev_deframer.push_dev(bits.data_ptr(), cap)
            assert dev_deframer.result() == ended and dev_deframer.stats() == deframer.stats()
    assert [len(s) for s in seen] == [1, 1] and seen[1][0][0] < cut, seen          # the second burst began in the first push
    assert [f[1] for f in frames] == payloads, (seen, [len(f[1]) for f in frames])
    assert dev_deframer.stats() == deframer.stats() and deframer.stats()[0] == len(payloads)


def test_process_pdus_without_midpoint_and_after_an_empty_push():
    rng = np.random.default_rng(41)
    burst = wm.g3ruh_burst(1)[0]
    x = np.concatenate([np.zeros(10, F32), burst, np.zeros(10, F32)])
    t = np.concatenate([np.zeros(10, F32), np.ones(len(burst), F32), np.zeros(10, F32)])
    pdus, w = rr.StreamToPdu(0.5, len(burst), 0), rr.Wpcr()
    rec = pdus.push(x, t)
    assert len(rec) == 1 and int(rec[0]["ok"]) == 1 and rec[0]["mid"] == 0 and int(rec[0]["nlow"]) == 0
    p, n_total = pdus.arena_dev()
    syms = torch.zeros(n_total, dtype=torch.float32, device="cuda")
    w.process_pdus(pdus, syms.data_ptr())
    res = w.results()
    (ref_syms, _), = rr.Wpcr().process([burst])
    assert len(res) == 1 and int(res[0]["nsyms"]) == len(ref_syms)
    got = syms.cpu().numpy()[int(rec[0]["start"]):int(rec[0]["start"]) + len(ref_syms)]
    assert np.array_equal(bits_of(got), bits_of(ref_syms))
    pdus.push(np.zeros(0, F32), np.zeros(0, F32))
    w.process_pdus(pdus, 0)
    assert len(w.results()) == 0 and w.pack(0, 0, 0)[0] == 0
    with pytest.raises(RuntimeError, match="not a stream_to_pdu handle"):
        w.process_pdus(w, 0)


@pytest.mark.parametrize("refused,message", [
    (lambda L: L.rr_stream_to_pdu_create(0.5, 512001, 0, 0), "max_size beyond 512000 samples"),
    (lambda L: L.rr_hdlc_framer_create(1 << 20, 0.0, 1.0), "unknown hdlc framer flags"),
])
def test_a_refused_create_does_not_leak_the_pending_options(refused, message):
    """rr_next_create_options belongs to ONE create call, also one that refuses before any device is touched.  On the raw
    library: the create proxy of the package arms the options again in front of every create and would hide a leak."""
    import ctypes as C
    from rustradio_amd._lib import BuildOpts, lib as raw_lib
    L = raw_lib()
    taps = np.hanning(301).astype(np.complex64)                    # non-decimating, a few hundred taps

    def fft_tile():
        h = L.rr_fir_c32_create(taps.ctypes.data_as(C.c_void_p), len(taps), 1, 0, 0.0, 0.0)
        assert h, rr.last_error()
        tile = L.rr_fir_fft_tile(h)
        L.rr_block_destroy(h)
        return tile

    assert L.rr_next_create_options(None) == 0
    assert fft_tile() > 0                                          # the default at this length: FFT tiles
    o = BuildOpts()
    o.fir_path = 1                                                 # RR_PATH_DIRECT
    assert L.rr_next_create_options(C.byref(o)) == 0
    assert fft_tile() == 0                                         # (the override does reach a create)
    assert fft_tile() > 0                                          # ... and only one
    assert L.rr_next_create_options(C.byref(o)) == 0
    assert not refused(L) and rr.last_error() == message
    assert fft_tile() > 0
