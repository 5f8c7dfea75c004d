"""GPU: rr_vco_create (Vco, src/vco.rs:9-37) and rr_fm_tx_create (RationalResampler -> Vco, examples/fm_tx.rs:84-91) against
the long-double truth of tests/tx_model.py within its derived bound, the sync / resampler window protocols call by call, the
carried phase, the reference's non-finite rule (through the fused block too), steps beyond 2 pi against the exact truth on a
dyadic grid, the kernel's own sincos phase by phase, and a loop-back through QuadratureDemod that needs no reference at all.
Windows of many tiles: tests/test_gpu_fm_tx_scale.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import rustradio_amd as rr
from harness import AGAIN, WAIT_DST, WAIT_SRC, drive_pageable, drive_registered, run_chain
from oracle import pyoracle as orc
from tx_model import (GRID_G, MX, bound, bound_steps, comp_err, fm_tx_truth, fm_tx_truth_grid, grid_noise, grid_signal,
                      sync_rule, truth_grid_error, vco_truth, vco_truth_grid)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 2048                              # the scan tile: VCO_T in rustradio_amd/csrc/kernels.hpp
K75 = 2.0 * math.pi * 75000 / 480000
K5 = 2.0 * math.pi * 5000 / 480000


def test_tile_constant_mirrors_the_kernel():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "kernels.hpp")).read()
    assert f"constexpr int VCO_T = {T};" in src


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def assert_within(got, truth, n_bound, what=""):
    e = comp_err(got, truth)
    print(f"{what}: {len(got)} outputs, worst component error {e:.4e}, bound {bound(n_bound):.4e}")
    assert e <= bound(n_bound), (what, e, bound(n_bound))


# ---- 1. lengths at every edge the scan has -----------------------------------------------------------------------------
_EDGES = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
_RANDOM = [int(v) for v in np.random.default_rng(1).integers(1, 5 * T + 1, 20)]


@pytest.mark.parametrize("n", _EDGES + _RANDOM)
def test_vco_lengths(n):
    a = noise(n, n)
    blk = rr.Vco(K75)
    assert blk.work(a, 0)[:4] == sync_rule(n, 0) == (WAIT_DST, 0, 0, 1)
    assert blk.work(a[:0], n)[:4] == sync_rule(0, n) == (WAIT_SRC, 0, 0, 1)
    st, c, p, need, y = blk.work(a, n)
    assert (st, c, p, need) == sync_rule(n, n) == (WAIT_SRC, n, n, 1)
    assert_within(y, vco_truth(a, K75), n, f"n={n}")


# ---- 2. the phase carried across calls ------------------------------------------------------------------------------------
def feed_sync(blk, a, windows):
    """windows = [(in_len, out_cap)]: every call's counts must be the sync rule's -> concatenated output"""
    pos, outs = 0, []
    for in_len, out_cap in windows:
        in_len = min(in_len, len(a) - pos)
        st, c, p, need, y = blk.work(a[pos:pos + in_len], out_cap)
        assert (st, c, p, need) == sync_rule(in_len, out_cap), (pos, in_len, out_cap)
        outs.append(y); pos += c
    assert pos == len(a)
    return np.concatenate(outs)


def test_vco_carry_across_calls():
    n = 6 * T
    a = noise(n, 2)
    rng = np.random.default_rng(3)
    windows, left, limited = [], n, 0
    while left:
        w = min(int(rng.integers(1, 3 * T + 1)), left)
        cap = w
        if rng.random() < 0.4:                    # output-limited: the rest of the window comes back in the next call
            cap = int(rng.integers(1, w + 1)); limited += cap < w
        if len(windows) % 3 == 1:
            windows += [(0, 100), (w, 0)]         # calls that move nothing must not move the phase
        windows.append((w, cap)); left -= min(w, cap)
    assert limited >= 2 and len(windows) >= 5 and (0, 100) in windows
    y = feed_sync(rr.Vco(K75), a, windows)
    assert_within(y, vco_truth(a, K75), n, f"{len(windows)} calls")


# ---- 3. wraps and drift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [K75, 6.0])
@pytest.mark.parametrize("dc", [1.0, -1.0])
def test_vco_wraps_and_drift(dc, k):
    n = 200_000
    a = np.full(n, dc, np.float32)
    cuts = [1, 4097, 30_000, 30_001, 77_777, 150_000]                             # 7 unequal calls
    sizes = np.diff([0] + cuts + [n])
    y = feed_sync(rr.Vco(k), a, [(int(s), 512_000) for s in sizes])
    assert_within(y, vco_truth(a, k), n, f"dc={dc} k={k}")


# ---- 4. non-finite samples ---------------------------------------------------------------------------------------------------
_N1 = 3 * T + 17


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("p", [0, 5, T - 1, T, 2 * T + 3, _N1 - 1])
def test_vco_non_finite(bad, p):
    a = noise(_N1, 4)
    a[p] = bad
    blk = rr.Vco(K75)
    y = blk.work(a, _N1)[4]
    assert len(y) == _N1
    if p:
        assert_within(y[:p], vco_truth(a[:p], K75), p, f"before p={p}")
    later = [blk.work(noise(m, 5 + m), m)[4] for m in (700, T + 5)]               # two further calls, finite input
    for part in [y[p:]] + later:
        assert len(part) and np.all(np.isnan(part.real)) and np.all(np.isnan(part.imag))


# ---- 4b. steps beyond 2 pi: the kernel takes whole turns out of the step, the reference lets the phase grow ------------------------
def _grid_signal(sig, n, seed):
    return grid_noise(n, seed)[0] if sig == "noise" else np.full(n, (1 << GRID_G) if sig == "dc+1" else -(1 << GRID_G), np.int64)


@pytest.mark.parametrize("sig", ["noise", "dc+1", "dc-1"])
@pytest.mark.parametrize("k", [10.0, 4.0 * math.pi, 13.0, 100.0, 1e4, 1e6, -1e6])   # 2 MX = 4 pi = 12.566...: either side of it
def test_vco_large_steps(k, sig):
    n = 3 * T + 17
    q = _grid_signal(sig, n, 11)
    y = feed_sync(rr.Vco(k), grid_signal(q), [(700, 700), (2 * T + 5, 2 * T + 5), (n, n)])
    e, b = comp_err(y, vco_truth_grid(q, GRID_G, k)), bound_steps(n, abs(k))
    print(f"large steps {sig} k={k}: {n} outputs, worst component error {e:.4e}, bound_steps {b:.4e}")
    assert truth_grid_error(n, k) <= 0.01 * b
    assert e <= b, (sig, k, e, b)


@pytest.mark.parametrize("sig", ["noise", "dc+1", "dc-1"])
def test_vco_absurd_k(sig):
    """k = 1e300: what is left of such a step after the whole turns is noise, so there is no truth.  Properties only."""
    n = 3 * T + 17
    blk = rr.Vco(1e300)
    y = feed_sync(blk, grid_signal(_grid_signal(sig, n, 12)), [(700, 700), (2 * T + 5, 2 * T + 5), (n, n)])
    assert len(y) == n and np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))
    d = float(np.max(np.abs(y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2 - 1.0)))
    print(f"k=1e300 {sig}: | re^2 + im^2 - 1 | <= {d:.4e}, allowed {2.0 ** -22:.4e}")
    assert d <= 2.0 ** -22
    st, c, p, need, y2 = blk.work(noise(T + 5, 13), 900)                          # an output-limited call afterwards
    assert (st, c, p, need) == sync_rule(T + 5, 900) == (WAIT_DST, 900, 900, 1) and len(y2) == 900


# ---- 4c. the kernel's own sincos, phase by phase -----------------------------------------------------------------------------------
def _edge_phases():
    ph = []
    for q in range(-8, 9):                        # every multiple of pi / 4 in [-MX, MX] and its neighbours: the quadrant switches
        c = q * (math.pi / 4)                     # (the f64 nearest to q pi / 4: pi / 4 is a power of two times f64 pi)
        up, dn = c, c
        ph.append(c)
        for _ in range(3):
            up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
            ph += [up, dn]
    assert MX in ph and float(np.nextafter(MX, np.inf)) in ph and float(np.nextafter(-MX, 0.0)) in ph   # the ends, inside and outside
    ph += [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -27, -2.0 ** -27]
    ph += np.random.default_rng(14).uniform(-MX, MX, 64).tolist()
    return ph


def test_vco_sincos_edges():
    """Vco(p) on the one sample 1.0 hands exactly the f64 p to the kernel's sincos: the phase starts at 0 and p * 1.0 = p.
    Truth: long-double sin / cos of that phase after the reference's one wrap (vco.rs:27-32; p - MX is exact there)."""
    ld = np.longdouble
    phases = _edge_phases()
    assert 180 <= len(phases) <= 260
    one = np.ones(1, np.float32)
    worst, quadrants = 0.0, set()
    for p in phases:
        st, c, n, need, y = rr.Vco(p).work(one, 1)
        assert (st, c, n, need) == sync_rule(1, 1) and len(y) == 1
        w = p - MX if p > MX else p + MX if p < -MX else p
        assert abs(w) <= MX
        quadrants.add(int(np.rint(w / (math.pi / 2))))
        e = max(abs(float(ld(y[0].real) - np.sin(ld(w)))), abs(float(ld(y[0].imag) - np.cos(ld(w)))))
        assert e <= bound(1), (p, w, y[0], e, bound(1))
        worst = max(worst, e)
    assert quadrants == set(range(-4, 5))
    print(f"sincos edges: {len(phases)} phases, worst component error {worst:.4e}, bound {bound(1):.4e}")


# ---- 4d. non-finite samples through the fused block ----------------------------------------------------------------------------------
def _oracle_stream(I, D, x):
    """the reference resampler's output for the whole of x"""
    yo = orc.RationalResampler(I, D, np.float32).work(x, len(x) * I // D + 2)[4]
    assert len(yo) == -(-len(x) * I // D)
    return yo


def _check_poisoned(y, yo, q, I, D, what):
    """vco.rs on the stream yo: the first non-finite sample poisons its own output and every later one, none before"""
    bad = np.flatnonzero(~np.isfinite(yo))
    first = int(bad[0]) if len(bad) else len(yo)
    assert len(y) == len(yo)
    if first:
        assert_within(y[:first], fm_tx_truth_grid(q, GRID_G, I, D, K75, first), first, f"{what}: clean before output {first}")
    assert np.all(np.isnan(y[first:].real)) and np.all(np.isnan(y[first:].imag)), what
    return first


def _non_finite_decimating():
    n_in = 3 * T + 11
    q, a = grid_noise(n_in, 15)
    for at, read in ((2, False), (3, True)):      # (m * 3) // 2 = 0, 1, 3, 4, 6, ...: index 2 is never read, index 3 is output 2
        x = a.copy(); x[at] = np.nan
        assert (at in ((np.arange(8) * 3) // 2).tolist()) == read
        yo = _oracle_stream(2, 3, x)
        st, c, p, need, y = rr.FmTx(2, 3, K75).work(x, len(yo) + 1)
        assert (st, c, p, need) == (WAIT_SRC, n_in, len(yo), 1)
        first = _check_poisoned(y, yo, q, 2, 3, f"2:3 NaN at {at}")
        assert first == (2 if read else len(yo))
        if not read:
            assert np.all(np.isfinite(y.real)) and np.all(np.isfinite(y.imag))


def _non_finite_interpolating():
    n_in = 3 * T + 11
    q, a = grid_noise(n_in, 16)
    x = a.copy(); x[5] = np.nan
    yo = _oracle_stream(10, 1, x)
    st, c, p, need, y = rr.FmTx(10, 1, K75).work(x, len(yo) + 1)
    assert (st, c, p, need) == (WAIT_SRC, n_in, 10 * n_in, 1)
    assert _check_poisoned(y, yo, q, 10, 1, "10:1 NaN at 5, one call") == 50
    # windows of 3 outputs: the NaN sample is the resampler's pending one from output 51 to 59, across three calls
    blk, ref = rr.FmTx(10, 1, K75), orc.RationalResampler(10, 1, np.float32)
    pos, outs, outs_o, nan_pending = 0, [], [], 0
    for cap in [3] * 25 + [10 * n_in]:
        got, want = blk.work(x[pos:], cap), ref.work(x[pos:], cap)
        assert got[:4] == want[:4], (pos, cap, got[:4], want[:4])
        nan_pending += cap == 3 and pos == 6 and bool(np.isnan(want[4][0]))    # sample 5 is consumed, its repeats still come
        outs.append(got[4]); outs_o.append(want[4]); pos += got[1]
    assert pos == n_in and nan_pending >= 2
    y3, yo3 = np.concatenate(outs), np.concatenate(outs_o)
    assert np.array_equal(yo3, yo, equal_nan=True)
    assert _check_poisoned(y3, yo3, q, 10, 1, "10:1 NaN at 5, windows of 3") == 50
    assert np.array_equal(np.isnan(y3.real), np.isnan(y.real)) and np.array_equal(np.isnan(y3.imag), np.isnan(y.imag))
    assert len(outs[-1]) > 3 * T and np.all(np.isnan(outs[-1].real))              # the later window read finite samples only


@pytest.mark.parametrize("ratio", ["2:3", "10:1"])
def test_fm_tx_non_finite(ratio):
    {"2:3": _non_finite_decimating, "10:1": _non_finite_interpolating}[ratio]()


# ---- 5. the fused block keeps the resampler's protocol ---------------------------------------------------------------------
RATIOS = [(10, 1), (480000, 48000), (3, 2), (2, 3), (1, 1), (7, 5)]


def drive_logged(blk, x, in_cap, out_cap):
    """one block under a Graph::run-style loop -> (outputs, [(status, consumed, produced, need, eof(true))])"""
    ring, pos, outs, log = np.zeros(0, blk.in_dtype), 0, [], []
    for _ in range(100_000):
        take = min(in_cap - len(ring), len(x) - pos)
        ring = np.concatenate([ring, x[pos:pos + take]]); pos += take
        st, c, p, need, out = blk.work(ring, out_cap)
        log.append((st, c, p, need, blk.eof(True)))
        ring = ring[c:]
        outs.append(out)
        if take == 0 and c == 0 and p == 0:
            return np.concatenate(outs), log
    raise AssertionError("no termination")


@pytest.mark.parametrize("out_cap", [1, 3, 64, 1000])
@pytest.mark.parametrize("ratio", RATIOS)
def test_fm_tx_protocol_is_the_resamplers(ratio, out_cap):
    I, D = ratio
    d = D // math.gcd(I, D)
    n_in = 40 * d if out_cap < 64 else 600 * d                                    # small windows: few samples, many calls
    x = noise(n_in, 6)
    in_cap = max(7, n_in // 3)
    y, log = drive_logged(rr.FmTx(I, D, K75), x, in_cap, out_cap)
    yo, log_o = drive_logged(orc.RationalResampler(I, D, np.float32), x, in_cap, out_cap)
    assert log == log_o
    if I > D and out_cap == 1:                    # the window fills after the first of a sample's repeats: pending, eof held back
        assert any(not e and st == WAIT_DST for st, _, _, _, e in log), "the pending path was not reached"
    assert len(y) == len(yo) == -(-n_in * I // D)
    assert_within(y, vco_truth(yo, K75), len(y), f"{I}:{D} out_cap={out_cap}")    # the oracle's resampled stream, modulated
    assert_within(y, fm_tx_truth(x, I, D, K75, len(y)), len(y), "index map")


def test_fm_tx_constructor_errors():
    with pytest.raises(ValueError, match="RationalResampler created using interp 0"):
        rr.FmTx(0, 1, K5)
    with pytest.raises(ValueError, match="RationalResampler created using deci 0"):
        rr.FmTx(1, 0, K5)
    for k in (float("nan"), float("inf"), -0.0, 1e300):                           # any k is accepted, as in the reference
        rr.Vco(k); rr.FmTx(3, 2, k)


# ---- 6. the fused block's samples ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RATIOS)
def test_fm_tx_samples(ratio):
    I, D = ratio
    n_in = 3 * T * D // I + 37
    x = noise(n_in, 7)
    st, c, p, need, y = rr.FmTx(I, D, K75).work(x, 8 * T)
    assert (st, c, need) == (WAIT_SRC, n_in, 1) and p == -(-n_in * I // D) and p > 3 * T
    assert_within(y, fm_tx_truth(x, I, D, K75, p), p, f"{I}:{D}")
    yu = run_chain([rr.RationalResampler(I, D, np.float32), rr.Vco(K75)], x)
    assert len(yu) == p
    d = max(np.max(np.abs(y.real.astype(np.float64) - yu.real)), np.max(np.abs(y.imag.astype(np.float64) - yu.imag)))
    print(f"{I}:{D} fused vs unfused {d:.4e}, allowed {2 * bound(p):.4e}")
    assert d <= 2 * bound(p)


# ---- 7. loop-back: FmTx -> QuadratureDemod gives the audio back, no reference needed -----------------------------------------
def test_loop_back_through_the_demodulator():
    k = 1.0
    audio = noise(2000, 8)
    y = run_chain([rr.FmTx(10, 1, k), rr.QuadratureDemod(1.0)], audio)
    a_r = np.repeat(audio, 10).astype(np.float64)
    assert len(y) == len(a_r) - 1
    # re = sin, im = cos: the stream is j e^(-j phase), so the demodulator sees MINUS the phase step
    e = float(np.max(np.abs(y.astype(np.float64) - (-k * a_r[1:]))))
    print(f"loop-back error {e:.4e}, allowed {2.0 ** -20:.4e}")
    assert e <= 2.0 ** -20


# ---- 8. plumbing ------------------------------------------------------------------------------------------------------------------
def test_names_sizes_and_tag_rules():
    v, f = rr.Vco(K5), rr.FmTx(10, 1, K5)
    p = C.c_size_t(0)
    assert rr.lib().rr_block_tag_rule(v._h, C.byref(p)) == 1 and p.value == 1     # RR_TAGS_FORWARD, position for position
    assert rr.lib().rr_block_tag_rule(f._h, C.byref(p)) == 0                      # RR_TAGS_DROP (the resampler's)
    assert v.name == "Vco" and f.name == "RationalResampler>Vco"
    for b in (v, f):
        assert rr.lib().rr_block_in_elem_size(b._h) == 4 and rr.lib().rr_block_out_elem_size(b._h) == 8
        assert rr.lib().rr_block_out_windows(b._h) == 1
        assert b.eof(True) and not b.eof(False)
    assert rr.lib().rr_abi_version() == 3


def through_device_streams(blk, x, stream_bytes):
    src, dst = rr.DeviceStream(np.float32, stream_bytes), rr.DeviceStream(np.complex64, 2 * stream_bytes)
    pos, outs = 0, []
    for _ in range(100_000):
        moved = src.push(x[pos:]); pos += moved
        while True:
            st, c, p, need = blk.work_streams(src, dst)
            moved += c + p
            if st != AGAIN or (c == 0 and p == 0):
                break
        y = dst.pop(); moved += len(y)
        outs.append(y)
        if moved == 0:
            return np.concatenate(outs)
    raise AssertionError("no termination")


@pytest.mark.parametrize("which", ["vco", "fm_tx"])
def test_device_streams(which):
    x = noise(3 * T + 5, 9)
    if which == "vco":
        y = through_device_streams(rr.Vco(K75), x, 4 * 1000)                      # 1000-sample rings: the carry, many times
        truth = vco_truth(x, K75)
    else:
        y = through_device_streams(rr.FmTx(3, 2, K75), x, 4 * 1000)
        truth = fm_tx_truth(x, 3, 2, K75, -(-len(x) * 3 // 2))
    assert len(y) == len(truth)
    assert_within(y, truth, len(y), which)


def test_registered_and_pageable_host_windows():
    x = noise(3 * T + 5, 10)
    y, log = drive_registered(rr, rr.Vco(K75), x, 1500, 1100)
    assert all(l == sync_rule(*w) for l, w in zip(log, _windows(len(x), 1500, 1100)))
    assert_within(y[0], vco_truth(x, K75), len(x), "registered")
    y, log = drive_pageable(rr.FmTx(7, 5, K75), x, 1500, 1100)
    n_out = -(-len(x) * 7 // 5)
    assert y.shape == (1, n_out)
    assert_within(y[0], fm_tx_truth(x, 7, 5, K75, n_out), n_out, "pageable")


def _windows(n, in_cap, out_cap):
    """the (in_len, out_cap) a sync block sees under harness.drive_registered"""
    have, pos = 0, 0
    while True:
        take = min(in_cap - have, n - pos); have += take; pos += take
        yield have, out_cap
        have -= min(have, out_cap)


# ---- 9. the C++ mirror -------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_fm_tx():
    exe = os.path.join(ROOT, "tests", "cpp", "test_fm_tx_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_fm_tx_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK")
