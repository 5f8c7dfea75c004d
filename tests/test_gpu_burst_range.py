"""GPU: the burst blocks (kernels_burst.hip) where tests/test_gpu_burst.py does not go — alpha from 2^-26 to 1 - 2^-24 within a
bound that stays at f32-ulp level there (burst_model.bound_gpu_any, against a long double truth), noise past one chunk of the
tile scan, the two rows of the Complex block held apart, both ends of the f32 range, and the edge list at its capacity, at a
value equal to the threshold, at odd thresholds and across calls nobody asked about."""
import numpy as np
import pytest

import rustradio_amd as rr
from burst_model import (bound_gpu, bound_gpu_any, bound_terms_any, burst_signal, coefficients, edges, iir_truth, iir_truth_ld,
                         ld_truth_error, mag2_f32)
from test_gpu_burst import T, bits, check_edges, feed_sync, fnoise, make_det, raw_edges, seam_signal, unfused
from tx_model import sync_rule

pytestmark = pytest.mark.gpu

LD = np.longdouble
_N1 = 3 * T + 17
FLT_MAX = float(np.finfo(np.float32).max)


def dc_noise(n, seed):
    """0.5 + U(-0.5, 0.5): the DC keeps |t| away from zero, so the cast term is what a result is held to"""
    return (0.5 + np.random.default_rng(seed).uniform(-0.5, 0.5, n)).astype(np.float32)


def split_windows(n, seed):
    """random_windows of tests/test_gpu_burst.py for any n >= 1: windows of 1 .. n / 3 + 1 samples, some output-limited,
    (0, 100) and (w, 0) calls in between -> (windows, the number of calls that move samples)"""
    rng = np.random.default_rng(seed)
    windows, pos, moving = [], 0, 0
    while pos < n:
        w = min(int(rng.integers(1, n // 3 + 2)), n - pos)
        cap = int(rng.integers(1, w + 1)) if rng.random() < 0.4 else w
        if len(windows) % 3 == 1:
            windows += [(0, 100), (w, 0)]
        windows.append((w, cap)); pos += min(w, cap); moving += 1
    return windows, moving


def assert_within_any(got, t, x, alpha, calls, what, vacuity=True):
    """got within bound_gpu_any of the long double truth t, whose own error is added in the open; prints the worst fraction of
    the allowance and holds the f64 term to under 1e-3 of the cast term, so that the check stays at the level of an f32 ulp"""
    assert len(got) == len(t) == len(x) and got.dtype == np.float32
    cast, f64 = bound_terms_any(t, x, alpha, calls)
    allow = cast + f64 + ld_truth_error(x, alpha)
    d = np.abs(got.astype(LD) - t).astype(np.float64)
    worst, ratio = float(np.max(d / allow)), float(np.median(f64 / cast))
    print(f"{what}: {len(got)} outputs, {calls} calls, worst error {float(np.max(d)):.3e}, {worst:.3f} of the bound, "
          f"f64 term / cast term {ratio:.2e}")
    assert np.all(d <= allow), (what, worst)
    if vacuity:
        assert ratio < 1e-3, (what, ratio)
    return worst


# ---- B1. alpha from 2^-26 to 1 - 2^-24 -------------------------------------------------------------------------------------------
_ALPHAS = [1e-3, 2.0 ** -12, 1e-5, 0.6 * 2.0 ** -24, 2.0 ** -26, 0.999, 1.0 - 2.0 ** -24]
_SWEEP = {}


def sweep_case(alpha, n):
    if (alpha, n) not in _SWEEP:
        x = dc_noise(n, 1000 + n)
        t = iir_truth_ld(x, alpha)[0]
        x.setflags(write=False); t.setflags(write=False)
        _SWEEP[alpha, n] = (x, t)
    return _SWEEP[alpha, n]


@pytest.mark.parametrize("n", [1, 9, T - 1, T + 1, _N1])
@pytest.mark.parametrize("alpha", _ALPHAS, ids=lambda a: f"{a:.9g}")
def test_alpha_sweep_one_call(alpha, n):
    x, t = sweep_case(alpha, n)
    st, c, p, need, y = rr.SinglePoleIirFilter(alpha).work(x, n)
    assert (st, c, p, need) == sync_rule(n, n)
    assert_within_any(y, t, x, alpha, 1, f"alpha {alpha:.6g} n {n}")
    a, b = coefficients(alpha)
    if b == 1.0:                                                                   # the recurrence is a plain sum
        assert_within_any(y, LD(a) * np.cumsum(x.astype(LD)), x, alpha, 1, f"alpha {alpha:.6g} n {n} against a cumsum(x)")


@pytest.mark.parametrize("n", [1, 9, T - 1, T + 1, _N1])
@pytest.mark.parametrize("alpha", _ALPHAS, ids=lambda a: f"{a:.9g}")
def test_alpha_sweep_split(alpha, n):
    x, t = sweep_case(alpha, n)
    windows, moving = split_windows(n, n + 7)
    assert n < 9 or moving >= 3
    y = feed_sync(rr.SinglePoleIirFilter(alpha), x, windows)
    assert_within_any(y, t, x, alpha, moving, f"alpha {alpha:.6g} n {n} split")


# ---- B2. noise past one chunk of the tile scan ------------------------------------------------------------------------------------
_NS = 4096 * T + T + 5
_NS2 = T + 5
_SCALE = {}


def scale_float():
    """uniform(-1, 1) noise of one scan chunk, a tile and five samples through the Float block, then T + 5 more on the same
    handle -> (x, x2, y, y2), shared"""
    if not _SCALE:
        x, x2 = fnoise(_NS, 50), fnoise(_NS2, 51)
        blk = rr.SinglePoleIirFilter(0.01)
        st, c, p, need, y = blk.work(x, _NS)
        assert (st, c, p, need) == sync_rule(_NS, _NS)
        y2 = blk.work(x2, _NS2)[4]
        _SCALE.update(x=x, x2=x2, y=y, y2=y2)
    return _SCALE["x"], _SCALE["x2"], _SCALE["y"], _SCALE["y2"]


def test_noise_past_one_scan_chunk():
    """every tile response of the chunk is different, so a swapped or shifted tile, or a wrong power in the chunk scan, shows;
    the second call starts from what a window of more than one chunk carried out"""
    alpha = 0.01
    x, x2, y, y2 = scale_float()
    t, prev = np.empty(_NS), 0.0
    for i in range(0, _NS, 1 << 20):                                               # the f64 fold, a slice at a time
        t[i:i + (1 << 20)], prev = iir_truth(x[i:i + (1 << 20)], alpha, prev)
    for got, want, X, what in ((y, t, float(np.max(np.abs(x))), "first call"),
                               (y2, iir_truth(x2, alpha, prev)[0], max(float(np.max(np.abs(x))), float(np.max(np.abs(x2)))), "second call")):
        d = np.abs(got.astype(np.float64) - want)
        b = bound_gpu(want, X, alpha)
        print(f"noise, alpha {alpha}, {what}: {len(got)} samples, worst error {float(np.max(d)):.3e}, {float(np.max(d / b)):.3f} of the bound")
        assert len(got) == len(want) and np.all(d <= b)


def test_complex_rows_past_one_scan_chunk():
    """the Complex block is two rows of the same launches: bit for bit what two Float blocks give for the two components"""
    xr, xr2, yr, yr2 = scale_float()
    xi, xi2 = fnoise(_NS, 52), fnoise(_NS2, 53)
    fi = rr.SinglePoleIirFilter(0.01)
    yi, yi2 = fi.work(xi, _NS)[4], fi.work(xi2, _NS2)[4]
    blk = rr.SinglePoleIirFilter(0.01, np.complex64)
    for re, im, wr, wi in ((xr, xi, yr, yi), (xr2, xi2, yr2, yi2)):
        z = np.empty(len(re), np.complex64)
        z.real, z.imag = re, im
        st, c, p, need, y = blk.work(z, len(z))
        assert (st, c, p, need) == sync_rule(len(z), len(z))
        assert np.array_equal(bits(y.real), bits(wr)) and np.array_equal(bits(y.imag), bits(wi))


# ---- B3. the two rows of the Complex block never meet -----------------------------------------------------------------------------
def run_parts(blk, z, split):
    parts = [z] if split is None else [z[:split], z[split:]]
    return np.concatenate([blk.work(part, len(part))[4] for part in parts if len(part)])


@pytest.mark.parametrize("two_calls", [False, True], ids=["one-call", "split-behind-p"])
@pytest.mark.parametrize("p", [0, T - 1, T, 2 * T + 3])
@pytest.mark.parametrize("bad,row", [(float("nan"), 0), (float("inf"), 1)], ids=["nan-in-re", "inf-in-im"])
def test_rows_are_independent(bad, row, p, two_calls):
    rng = np.random.default_rng(60)
    z = (rng.standard_normal(_N1) + 1j * rng.standard_normal(_N1)).astype(np.complex64)
    split = p + 1 if two_calls else None
    clean = run_parts(rr.SinglePoleIirFilter(0.3, np.complex64), z, split)
    zb = z.copy()
    zb.view(np.float32)[2 * p + row] = bad
    got = run_parts(rr.SinglePoleIirFilter(0.3, np.complex64), zb, split)
    assert len(got) == len(clean) == _N1 and np.all(np.isfinite(clean.view(np.float32)))
    comp = lambda a, r: np.ascontiguousarray(a.view(np.float32)[r::2])
    assert np.array_equal(bits(comp(got, 1 - row)), bits(comp(clean, 1 - row)))    # the other component: untouched, bit for bit
    hit = comp(got, row)
    assert np.array_equal(bits(hit[:p]), bits(comp(clean, row)[:p]))
    assert np.all(np.isnan(hit[p:])) if np.isnan(bad) else np.all(~np.isfinite(hit[p:]))


# ---- B4. the ends of the f32 range -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [3, T - 100], ids=["in-tile", "across-the-seam"])
def test_decay_through_the_subnormals(at):
    """alpha 0.5 after one sample of 1.0: 2^-k exactly, in f64 and in the tables, so the f32 delivered is the truth cast once,
    bit for bit — through the subnormals (2^-127 .. 2^-149), the tie 2^-150 that rounds to zero, and +0.0 from there on"""
    n = T + 300
    x = np.zeros(n, np.float32)
    x[at] = 1.0
    want = iir_truth(x, 0.5)[0].astype(np.float32)
    k = np.arange(n - at)
    assert np.array_equal(want[at:at + 149], (2.0 ** -(k[:149] + 1.0)).astype(np.float32)) and not want[at + 149:].any()
    assert np.count_nonzero((want > 0) & (want < np.finfo(np.float32).tiny)) == 23
    y = rr.SinglePoleIirFilter(0.5).work(x, n)[4]
    assert np.array_equal(bits(y), bits(want))
    for cut in (at + 130, at + 149):                                               # the carried y is a subnormal of f32; then 2^-150
        blk = rr.SinglePoleIirFilter(0.5)
        y = np.concatenate([blk.work(x[:cut], cut)[4], blk.work(x[cut:], n - cut)[4]])
        assert np.array_equal(bits(y), bits(want)), cut


@pytest.mark.parametrize("alpha", [0.3, 1e-3, 0.999])
def test_subnormal_inputs(alpha):
    rng = np.random.default_rng(61)
    x = (rng.integers(-(2 ** 23) + 1, 2 ** 23, _N1).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert np.all(np.abs(x) < np.finfo(np.float32).tiny) and np.count_nonzero(x) > _N1 - 10
    t = iir_truth_ld(x, alpha)[0]
    y = rr.SinglePoleIirFilter(alpha).work(x, _N1)[4]
    assert_within_any(y, t, x, alpha, 1, f"subnormal inputs, alpha {alpha}", vacuity=False)
    assert np.count_nonzero(y) > _N1 // 2 and np.all(np.abs(y) < np.finfo(np.float32).tiny)
    assert np.all(bound_gpu_any(t, x, alpha) < 2.0 ** -149)                        # under one ulp: the nearest or its neighbour


def test_flt_max_inputs():
    x = np.full(_N1, FLT_MAX, np.float32)
    x[1::2] = -FLT_MAX
    t = iir_truth_ld(x, 0.3)[0]
    for windows, calls in (([(_N1, _N1)], 1), split_windows(_N1, 62)):
        y = feed_sync(rr.SinglePoleIirFilter(0.3), x, windows)
        assert np.all(np.isfinite(y))
        assert_within_any(y, t, x, 0.3, calls, "+-FLT_MAX")
    y = rr.SinglePoleIirFilter(1.0).work(x, _N1)[4]
    assert np.array_equal(bits(y), bits(x))


def test_mag2_products_that_underflow():
    rng = np.random.default_rng(63)
    n = _N1
    mag = 10.0 ** rng.uniform(-23.0, -20.0, (2, n)) * rng.choice([-1.0, 1.0], (2, n))
    z = (mag[0] + 1j * mag[1]).astype(np.complex64)
    want = mag2_f32(z)
    tiny = np.finfo(np.float32).tiny
    assert np.count_nonzero(want == 0) > 100 and np.count_nonzero((want > 0) & (want < tiny)) > n // 2
    y = rr.ComplexToMag2().work(z, n)[4]
    assert np.array_equal(bits(y), bits(want))
    y = rr.BurstDetector(1.0, 1e-3).work(z, n)[4]                                  # the same loader inside the scan kernels
    assert np.array_equal(bits(y), bits(want))


def test_detector_threshold_in_the_subnormals():
    n, thr = T + 300, 2.0 ** -140
    z = np.zeros(n, np.complex64)
    z[3] = 1.0
    det = make_det(0.5, thr)
    y = det.work(z, n)[4]
    assert np.array_equal(bits(y), bits(iir_truth(mag2_f32(z), 0.5)[0].astype(np.float32)))
    assert check_edges(det, y, False) == 2
    pos, val = det.edges()
    assert list(zip(pos.tolist(), val.tolist())) == [(3, True), (3 + 139, False)]   # 2^-(k+1) > 2^-140 up to k = 138


# ---- B5. the edge list ----------------------------------------------------------------------------------------------------------------
def edge_pairs(det):
    pos, val = det.edges()
    return list(zip(pos.tolist(), val.tolist()))


def test_every_sample_an_edge():
    """the list's capacity is one slot per sample, and here every sample needs its slot: 64 edges in every wave's ballot, every
    seam an edge, in one call and with the flag carried across calls of T, 1, T + 1 and the rest"""
    n = _N1
    z = np.zeros(n, np.complex64)
    z[0::2] = 0.25
    want = [(i, i % 2 == 0) for i in range(n)]
    det = make_det(1.0, 0.03)
    y = det.work(z, n)[4]
    rc, pos, val, total = raw_edges(det, 5)                                        # fewer than there are, first
    assert rc == 0 and total == n and list(zip(pos.tolist(), val.astype(bool).tolist())) == want[:5]
    assert check_edges(det, y, False) == n and edge_pairs(det) == want
    det, off, last, got = make_det(1.0, 0.03), 0, False, []
    for m in (T, 1, T + 1, n - 2 * T - 2):
        y = det.work(z[off:off + m], m)[4]
        assert check_edges(det, y, last) == m
        got += [(p + off, v) for p, v in edge_pairs(det)]
        off += m; last = bool(y[-1] > np.float32(0.03))
    assert off == n and got == want


def test_a_value_equal_to_the_threshold_is_not_above_it():
    z, want = seam_signal()
    det = make_det(1.0, 0.0625)                                                    # the envelope is 0.0625 or 0, exactly
    y = det.work(z, len(z))[4]
    assert np.count_nonzero(y == np.float32(0.0625)) > T and check_edges(det, y, False) == 0
    det = make_det(1.0, float(np.nextafter(np.float32(0.0625), np.float32(0))))     # one ulp lower: all of them
    y = det.work(z, len(z))[4]
    assert check_edges(det, y, False) == len(want) and edge_pairs(det) == want


def test_thresholds_of_zero_and_below():
    zeros, noise = np.zeros(T + 9, np.complex64), burst_signal(_N1, 5)
    det = make_det(0.3, 0.0)
    y = det.work(zeros, len(zeros))[4]
    assert not y.any() and check_edges(det, y, False) == 0                         # 0 > 0 is false
    for thr in (-1.0, float("-inf")):                                              # always above: one rising edge, once
        det = make_det(0.3, thr)
        for k, part in enumerate((zeros, noise, noise[:1], zeros)):
            y = det.work(part, len(part))[4]
            assert check_edges(det, y, k > 0) == (1 if k == 0 else 0)
            assert edge_pairs(det) == ([(0, True)] if k == 0 else [])


def test_subnormal_threshold():
    thr = 2.0 ** -149
    zeros = np.zeros(T + 9, np.complex64)
    det = make_det(0.5, thr)
    y = det.work(zeros, len(zeros))[4]
    assert check_edges(det, y, False) == 0
    z = zeros.copy()
    z[5] = 2.0 ** -74                                                              # x = 2^-148, y = 2^-149 = the threshold, then 0
    y = det.work(z, len(z))[4]
    assert y[5] == np.float32(thr) and np.count_nonzero(y) == 1 and check_edges(det, y, False) == 0
    det = make_det(1.0, thr)
    z[T] = 2.0 ** -74                                                              # alpha 1: 2^-148, above it, at 5 and at the seam
    y = det.work(z, len(z))[4]
    assert check_edges(det, y, False) == 4 and edge_pairs(det) == [(5, True), (6, False), (T, True), (T + 1, False)]


def test_edges_are_those_of_the_last_moving_call():
    """three calls that move samples and no edges() in between: the list is the third call's, window-relative, with the flag
    the second call left — the counters are ping-pong, each call zeroing the next one's"""
    rng = np.random.default_rng(64)
    z = (rng.standard_normal(5 * T) + 1j * rng.standard_normal(5 * T)).astype(np.complex64)
    thr = float(np.median(unfused(z, 0.5)))
    det = make_det(0.5, thr)
    y1 = det.work(z[:_N1], _N1)[4]
    y2 = det.work(z[_N1:_N1 + 700], 700)[4]
    y3 = det.work(z[_N1 + 700:], len(z))[4]
    assert len(edges(y1, thr)[0]) > len(edges(y3, thr)[0]) > len(edges(y2, thr)[0]) > 100
    assert check_edges(det, y3, bool(y2[-1] > np.float32(thr))) > 100
    assert det.work(z[:0], 10)[2] == 0 and edge_pairs(det) == []                   # and a call that moves nothing has none


# ---- B6. detector fuzz -----------------------------------------------------------------------------------------------------------------
_FUZZ_ALPHAS = [1e-4, 1e-3, 0.01, 0.1, 0.5, 0.97]


@pytest.mark.parametrize("seed", range(24))
def test_detector_fuzz(seed):
    rng = np.random.default_rng(7000 + seed)
    alpha = _FUZZ_ALPHAS[int(rng.integers(len(_FUZZ_ALPHAS)))]
    n = (1, T + 1, 6 * T)[seed] if seed < 3 else int(rng.integers(1, 6 * T + 1))
    z = burst_signal(n, 100 + seed)
    thr = float(np.median(unfused(z, alpha))) if seed % 2 == 0 else 1e-3
    windows, moving = split_windows(n, 200 + seed)
    det, m2, iir = make_det(alpha, thr), rr.ComplexToMag2(), rr.SinglePoleIirFilter(alpha)
    pos, last, outs, nedges = 0, False, [], 0
    for w, cap in windows:
        part = z[pos:pos + min(w, n - pos)]
        st, c, p, need, y = det.work(part, cap)
        assert (st, c, p, need) == sync_rule(len(part), cap)
        if p == 0:
            assert len(det.edges()[0]) == 0
            continue
        nedges += check_edges(det, y, last, f"seed {seed} window at {pos}")        # invariant E on the call's own output
        xs = m2.work(part, cap)[4]
        assert np.array_equal(bits(y), bits(iir.work(xs, cap)[4])), (seed, pos)    # fused is unfused, window for window
        outs.append(y); pos += c; last = bool(y[-1] > np.float32(thr))
    assert pos == n
    x = mag2_f32(z)
    worst = assert_within_any(np.concatenate(outs), iir_truth_ld(x, alpha)[0], x, alpha, moving,
                              f"fuzz seed {seed} alpha {alpha} n {n} thr {thr:.3e} edges {nedges}", vacuity=False)
    assert worst <= 1.0
