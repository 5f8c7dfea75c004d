"""GPU: rr_complex_to_mag2_create, rr_single_pole_iir_create and rr_burst_detector_create against the models of
tests/burst_model.py — ComplexToMag2 bit for bit, the f64 scan within its derived bound of the exact recurrence (and within
the sum of both bounds of the reference's f32 fold), the carried state, the non-finite rule, fused against unfused bit for
bit, and the edge list against the comparison of BurstTagger applied to the f32 values the block itself delivered.
Where the edge list is compared with the reference's fold, tests/test_burst_cpu.py proves the input has no ambiguous sample."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rustradio_amd as rr
from burst_model import (bound_gpu, bound_ref, burst_signal, edges, iir_ref_f32, iir_truth, iir_truth_const, mag2_f32)
from harness import AGAIN, WAIT_DST, WAIT_SRC
from tx_model import sync_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 2048                              # the scan tile: IIR_T in rustradio_amd/csrc/kernels.hpp


def test_tile_constant_mirrors_the_kernel():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "kernels.hpp")).read()
    assert f"constexpr int IIR_T = {T};" in src


_EDGES = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
_RANDOM = [int(v) for v in np.random.default_rng(1).integers(1, 5 * T + 1, 20)]


def cnoise(n, seed, sigma=1.0):
    rng = np.random.default_rng(seed)
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def fnoise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)     # mixed sign


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_sync_counts(blk, x):
    n = len(x)
    assert blk.work(x, 0)[:4] == sync_rule(n, 0) == (WAIT_DST, 0, 0, 1)
    assert blk.work(x[:0], n)[:4] == sync_rule(0, n) == (WAIT_SRC, 0, 0, 1)


def assert_within(got, t, X, alpha, what="", extra=0.0):
    assert len(got) == len(t)
    d = np.abs(got.astype(np.float64) - t)
    b = bound_gpu(t, X, alpha) + extra
    worst = float(np.max(d / b)) if len(d) else 0.0
    print(f"{what}: {len(got)} outputs, worst error {float(np.max(d)) if len(d) else 0.0:.3e}, {worst:.3f} of the bound")
    assert np.all(d <= b), (what, worst)


def feed_sync(blk, x, windows, after=None):
    """windows = [(in_len, out_cap)]: every call's counts must be the sync rule's -> concatenated output"""
    pos, outs = 0, []
    for in_len, out_cap in windows:
        in_len = min(in_len, len(x) - pos)
        st, c, p, need, y = blk.work(x[pos:pos + in_len], out_cap)
        assert (st, c, p, need) == sync_rule(in_len, out_cap), (pos, in_len, out_cap)
        if after is not None:
            after(pos, y)
        outs.append(y); pos += c
    assert pos == len(x)
    return np.concatenate(outs)


def random_windows(n, seed, cuts=()):
    """windows of 1 .. 3 T samples over n, some output-limited, (0, 100) and (w, 0) calls in between; `cuts`: forced ends"""
    rng = np.random.default_rng(seed)
    windows, pos, limited, cuts = [], 0, 0, sorted(cuts)
    while pos < n:
        w = min(int(rng.integers(1, 3 * T + 1)), n - pos)
        cap = w
        if rng.random() < 0.4:
            cap = int(rng.integers(1, w + 1)); limited += cap < w
        for c in cuts:
            if pos < c < pos + min(w, cap):
                cap = c - pos
        if len(windows) % 3 == 1:
            windows += [(0, 100), (w, 0)]
        windows.append((w, cap)); pos += min(w, cap)
    assert limited >= 1 and (0, 100) in windows
    return windows


# ---- 1. ComplexToMag2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", _EDGES + _RANDOM)
def test_mag2_lengths(n):
    z = cnoise(n, n)
    blk = rr.ComplexToMag2()
    check_sync_counts(blk, z)
    st, c, p, need, y = blk.work(z, n)
    assert (st, c, p, need) == sync_rule(n, n)
    assert bits(y).tolist() == bits(mag2_f32(z)).tolist()
    st, c, p, need, y = blk.work(z, max(1, n // 2))                                # output-limited
    assert (st, c, p, need) == sync_rule(n, max(1, n // 2)) and np.array_equal(y, mag2_f32(z)[:p])


def test_mag2_non_finite():
    z = cnoise(300, 2)
    nan, inf = float("nan"), float("inf")
    z[3] = complex(nan, 1.0); z[64] = complex(2.0, nan); z[100] = complex(inf, 1.0); z[101] = complex(-inf, inf)
    z[255] = complex(nan, inf); z[299] = complex(1e30, 1e30)                       # overflow: +Inf
    y = rr.ComplexToMag2().work(z, 300)[4]
    assert np.array_equal(y, mag2_f32(z), equal_nan=True)
    assert np.isnan(y[3]) and np.isnan(y[64]) and y[100] == inf and y[101] == inf and np.isnan(y[255]) and y[299] == inf
    assert np.all(np.isfinite(np.delete(y, [3, 64, 100, 101, 255, 299])))


# ---- 2. SinglePoleIirFilter, f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.01, 0.3])
@pytest.mark.parametrize("n", _EDGES + _RANDOM)
def test_iir_lengths(n, alpha):
    x = fnoise(n, n)
    X = float(np.max(np.abs(x)))
    blk = rr.SinglePoleIirFilter(alpha)
    check_sync_counts(blk, x)
    st, c, p, need, y = blk.work(x, n)
    assert (st, c, p, need) == sync_rule(n, n)
    t = iir_truth(x, alpha)[0]
    assert_within(y, t, X, alpha, f"n={n} alpha={alpha}")
    ref = iir_ref_f32(x, alpha)[0].astype(np.float64)
    assert np.all(np.abs(y.astype(np.float64) - ref) <= bound_gpu(t, X, alpha) + bound_ref(X, alpha))


# ---- 3. Complex: two independent recurrences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, T - 1, T + 1, 3 * T + 17])
def test_iir_complex_is_two_float_blocks(n):
    z = cnoise(n, 30 + n)
    blk = rr.SinglePoleIirFilter(0.3, np.complex64)
    check_sync_counts(blk, z)
    a, b = n // 3 + 1, n - (n // 3 + 1)
    fr, fi = rr.SinglePoleIirFilter(0.3), rr.SinglePoleIirFilter(0.3)
    for part in (z[:a], z[a:]):                                                    # two calls: the two carried values too
        if not len(part):
            continue
        st, c, p, need, y = blk.work(part, len(part))
        assert (st, c, p, need) == sync_rule(len(part), len(part))
        yr = fr.work(np.ascontiguousarray(part.real), len(part))[4]
        yi = fi.work(np.ascontiguousarray(part.imag), len(part))[4]
        assert bits(y.real).tolist() == bits(yr).tolist() and bits(y.imag).tolist() == bits(yi).tolist()
    assert a + b == n


# ---- 4. the state carried across calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.01, 0.3])
def test_iir_carry_across_calls(alpha):
    """Within the bound of the truth of the WHOLE stream.  Not bit-identical to one call of 6 T samples: the tile grid
    restarts at every window, so a sample's predecessors reach it through a different tree of combinations, each rounded once
    in f64; the bound holds for every tree."""
    n = 6 * T
    x = fnoise(n, 4)
    windows = random_windows(n, 5)
    assert len(windows) >= 5
    y = feed_sync(rr.SinglePoleIirFilter(alpha), x, windows)
    assert_within(y, iir_truth(x, alpha)[0], float(np.max(np.abs(x))), alpha, f"{len(windows)} calls, alpha {alpha}")


# ---- 5. alpha 0 and alpha 1 ----------------------------------------------------------------------------------------------------------
def test_alpha_zero_and_one():
    x = fnoise(3 * T + 8, 6)
    x[x == 0] = 0.5
    z = rr.SinglePoleIirFilter(0.0)
    for part in (x[:T + 5], x[T + 5:]):
        y = z.work(part, len(part))[4]
        assert len(y) == len(part) and bits(y).tolist() == [0] * len(part)       # exactly +0.0f
    one = rr.SinglePoleIirFilter(1.0)
    for part in (x[:T + 5], x[T + 5:]):
        y = one.work(part, len(part))[4]
        assert bits(y).tolist() == bits(part).tolist()
    zc = cnoise(T + 9, 7)
    y = rr.SinglePoleIirFilter(1.0, np.complex64).work(zc, len(zc))[4]
    assert bits(y.view(np.float32)).tolist() == bits(zc.view(np.float32)).tolist()


# ---- 6. non-finite samples --------------------------------------------------------------------------------------------------------------
_N1 = 3 * T + 17


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("p", [0, 5, T - 1, T, 2 * T + 3, _N1 - 1])
def test_iir_non_finite(bad, p):
    alpha = 0.3
    x = fnoise(_N1, 8)
    x[p] = bad
    blk = rr.SinglePoleIirFilter(alpha)
    y = blk.work(x, _N1)[4]
    assert len(y) == _N1
    if p:
        assert_within(y[:p], iir_truth(x[:p], alpha)[0], 1.0, alpha, f"before p={p}")
    later = [blk.work(fnoise(m, 9 + m), m)[4] for m in (700, T + 5)]               # two further calls, finite input
    if np.isnan(bad):
        for part in [y[p:]] + later:
            assert len(part) and np.all(np.isnan(part))
    else:
        assert np.all(~np.isfinite(y[p:]))                                        # Inf or NaN: not pinned
        assert np.all(~np.isfinite(later[0]))                                     # b^700 has not underflowed: still poisoned


@pytest.mark.parametrize("p", [0, T, _N1 - 1])
def test_detector_nan_sample(p):
    z = cnoise(_N1, 10, 0.1)
    z[p] = complex(float("nan"), 0.0)
    det = rr.BurstDetector(0.3, 1e-3)
    y = det.work(z, _N1)[4]
    assert np.all(np.isfinite(y[:p])) and np.all(np.isnan(y[p:]))
    pos, val = det.edges()
    em = edges(y, 1e-3)
    assert np.array_equal(pos, em[0]) and np.array_equal(val, em[1])              # a NaN envelope is never above the threshold
    y2 = det.work(cnoise(500, 11, 0.1), 500)[4]
    assert np.all(np.isnan(y2)) and len(det.edges()[0]) == 0


# ---- 7. fused equals unfused ----------------------------------------------------------------------------------------------------------------
def unfused(z, alpha):
    x = rr.ComplexToMag2().work(z, len(z))[4]
    return rr.SinglePoleIirFilter(alpha).work(x, len(x))[4]


@pytest.mark.parametrize("n", [60000, T - 1, T + 1, 3 * T + 17])
def test_fused_envelope_is_the_unfused_one(n):
    z = burst_signal(n, 7) if n == 60000 else cnoise(n, 12, 0.05)
    det = rr.BurstDetector(0.1, 1e-3)
    check_sync_counts(det, z)
    st, c, p, need, y = det.work(z, n)
    assert (st, c, p, need) == sync_rule(n, n)
    assert bits(y).tolist() == bits(unfused(z, 0.1)).tolist()
    x = mag2_f32(z)
    assert_within(y, iir_truth(x, 0.1)[0], float(np.max(x)), 0.1, f"detector n={n}")


# ---- 8. invariant (E): the edges are those of the f32 values the block delivered ---------------------------------------------------------
def check_edges(det, y, last, where=""):
    pos, val = det.edges()
    em = edges(y, det_thr(det), last)
    assert pos.dtype == np.uint64 and val.dtype == bool
    assert np.array_equal(pos, em[0]) and np.array_equal(val, em[1]), where
    assert np.all(np.diff(pos.astype(np.int64)) > 0)
    if len(val):
        assert val[0] == (not last) and np.all(val[1:] != val[:-1])
    return len(pos)


_THR = {}


def det_thr(det):
    return _THR[id(det)]


def make_det(alpha, thr):
    det = rr.BurstDetector(alpha, thr)
    _THR[id(det)] = thr
    return det


def test_edges_hovering_around_the_threshold():
    n = 6 * T
    z = cnoise(n, 13)
    env = unfused(z, 0.5)
    thr = float(np.median(env))
    whole = edges(env, thr)[0]
    assert len(whole) > 2000
    cut = int(whole[len(whole) // 2])                                              # a window that ends right before an edge ...
    state = {"last": False, "count": 0, "calls": 0}
    det = make_det(0.5, thr)

    def after(pos, y):
        if len(y):
            state["count"] += check_edges(det, y, state["last"], f"window at {pos}")
            state["last"] = bool(y[-1] > np.float32(thr)); state["calls"] += 1
        else:
            assert len(det.edges()[0]) == 0                                        # a call that moved nothing has none
    windows = random_windows(n, 14, cuts=[cut, cut + 1])                           # ... and one that holds only that edge
    y = feed_sync(det, z, windows, after)
    print(f"{state['count']} edges over {state['calls']} calls, threshold {thr:.4f}")
    assert state["count"] > 2000
    x = mag2_f32(z)
    assert_within(y, iir_truth(x, 0.5)[0], float(np.max(x)), 0.5, "hover")


# ---- 9. seams, with no tolerance at all -----------------------------------------------------------------------------------------------------
def seam_signal():
    n = 2 * T + 100
    toggles = [0, 1, 7, 8, 63, 64, T - 1, T, T + 1, 2 * T - 1, 2 * T, n - 1]
    z = np.zeros(n, np.complex64)
    for on, off in zip(toggles[0::2], toggles[1::2]):
        z[on:off] = 0.25
    return z, [(p, i % 2 == 0) for i, p in enumerate(toggles)]


@pytest.mark.parametrize("split", [None, T, T + 1])
def test_seams_exact(split):
    """alpha 1: the envelope is x = 0.0625 or 0 exactly, so every crossing is where the signal puts it"""
    z, want = seam_signal()
    det = make_det(1.0, 0.03)
    parts = [z] if split is None else [z[:split], z[split:]]
    got, off, last = [], 0, False
    for part in parts:
        y = det.work(part, len(part))[4]
        assert bits(y).tolist() == bits(mag2_f32(part)).tolist()
        check_edges(det, y, last)
        pos, val = det.edges()
        got += [(int(p) + off, bool(v)) for p, v in zip(pos, val)]
        off += len(part); last = bool(y[-1] > np.float32(0.03))
    assert got == want


# ---- 10. against the reference's fold ---------------------------------------------------------------------------------------------------------
_REF = {}


def _ref_edges(alpha):
    if alpha not in _REF:
        z = burst_signal(60000, 7)
        _REF[alpha] = (z, edges(iir_ref_f32(mag2_f32(z), alpha)[0], 1e-3))
    return _REF[alpha]


@pytest.mark.parametrize("alpha", [0.5, 0.1, 0.01])
def test_edges_are_the_references(alpha):
    """legitimate because tests/test_burst_cpu.py proves that this input has no ambiguous sample at these alphas"""
    z, (rpos, rval) = _ref_edges(alpha)
    assert len(rpos) == (6 if alpha == 0.01 else 8)
    for sizes in ([60000], [1, 4999, 2048, 12952, 10001, 29000, 999]):
        assert sum(sizes) == 60000
        det, off, got = make_det(alpha, 1e-3), 0, []
        for s in sizes:
            y = det.work(z[off:off + s], s)[4]
            assert len(y) == s
            pos, val = det.edges()
            got += [(int(p) + off, bool(v)) for p, v in zip(pos, val)]
            off += s
        assert got == list(zip(rpos.tolist(), rval.tolist())), (alpha, len(sizes))


# ---- 11. scale: past one chunk of the tile scan and the grid-stride loop -----------------------------------------------------------------
def test_scale():
    n = 4096 * T + T + 5
    rng = np.random.default_rng(15)
    segs, left, on = [], n, False
    while left:
        l = min(int(rng.integers(1_000_000, 3_000_001)), left)
        segs.append((0.0625 if on else 0.0, l)); left -= l; on = not on
    z = np.concatenate([np.full(l, 0.25 if v else 0.0, np.complex64) for v, l in segs])
    alpha, thr = 0.01, 0.03
    t = iir_truth_const(segs, alpha)
    assert len(t) == n == len(z)
    b = bound_gpu(t, 0.0625, alpha)
    assert np.all(np.abs(t - float(np.float32(thr))) > b)                          # no sample the cast could put on either side
    det = make_det(alpha, thr)
    st, c, p, need, y = det.work(z, n)
    assert (st, c, p, need) == sync_rule(n, n)
    d = np.abs(y.astype(np.float64) - t)
    print(f"scale: {n} samples, {len(segs)} segments, worst error {float(np.max(d)):.3e}, {float(np.max(d / b)):.3f} of the bound")
    assert np.all(d <= b)
    pos, val = det.edges()
    em = edges(t.astype(np.float32), thr)
    assert np.array_equal(pos, em[0]) and np.array_equal(val, em[1]) and len(pos) == len(segs) - 1
    check_edges(det, y, False)


# ---- 12. retrieval ------------------------------------------------------------------------------------------------------------------------------
def raw_edges(blk, cap):
    pos, val, total = np.full(max(cap, 1), 2 ** 63, np.uint64), np.full(max(cap, 1), 9, np.uint8), C.c_size_t(0)
    rc = rr.lib().rr_burst_edges(blk._h, pos.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p), cap, C.byref(total))
    return rc, pos, val, total.value


def test_edge_retrieval():
    z, want = seam_signal()
    det = make_det(1.0, 0.03)
    det.work(z, len(z))
    rc, pos, val, total = raw_edges(det, 5)
    assert rc == 0 and total == len(want) == 12
    assert list(zip(pos.tolist(), val.astype(bool).tolist())) == want[:5]
    rc, pos, val, total = raw_edges(det, 40)                                       # more room than edges: the rest untouched
    assert rc == 0 and total == 12 and list(zip(pos[:12].tolist(), val[:12].astype(bool).tolist())) == want
    assert np.all(pos[12:] == 2 ** 63) and np.all(val[12:] == 9)
    for thr in (float("nan"), float("inf")):
        d = rr.BurstDetector(1.0, thr)
        d.work(z, len(z))
        assert len(d.edges()[0]) == 0
    for other in (rr.ComplexToMag2(), rr.SinglePoleIirFilter(0.5)):
        rc, _, _, _ = raw_edges(other, 4)
        assert rc == rr.ERR and "burst detector" in rr.last_error()


def test_a_call_that_moves_nothing_keeps_the_flag():
    det = make_det(1.0, 0.03)
    hi, lo = np.full(10, 0.25, np.complex64), np.zeros(10, np.complex64)
    det.work(hi, 10)
    assert [(int(p), bool(v)) for p, v in zip(*det.edges())] == [(0, True)]
    for inp, cap in ((hi[:0], 100), (hi, 0)):
        assert det.work(inp, cap)[:4] == sync_rule(len(inp), cap)
        assert len(det.edges()[0]) == 0
    det.work(hi, 10)                                                               # still above: no edge at 0
    assert len(det.edges()[0]) == 0
    det.work(lo, 10)
    assert [(int(p), bool(v)) for p, v in zip(*det.edges())] == [(0, False)]


def test_an_empty_call_between_two_windows_leaves_the_state_alone():
    """two windows of one tile plus one sample (the tile seam and the carried flag both in play), crossings at sample 0, at the
    seam and at the last sample; the first window ends above the threshold, so a flag read from the wrong half of its pair
    (false, as at the start) would move the second window's edge at sample 0"""
    hi, lo = np.complex64(0.25), np.complex64(0)
    w1 = np.array([hi] + [lo] * (T - 1) + [hi])
    w2 = np.array([lo] * T + [hi])
    want = [[(0, True), (1, False), (T, True)], [(0, False), (T, True)]]
    runs = []
    for empty in (False, True):
        det, got = make_det(0.5, 0.03), []
        for i, w in enumerate((w1, w2)):
            if empty and i == 1:
                assert det.work(w[:0], 100)[:4] == sync_rule(0, 100)
                assert len(det.edges()[0]) == 0
            st, c, p, need, y = det.work(w, len(w))
            assert (st, c, p, need) == sync_rule(len(w), len(w))
            got.append((bits(y).tolist(), [(int(a), bool(b)) for a, b in zip(*det.edges())]))
        runs.append(got)
    assert runs[0] == runs[1]
    assert [e for _, e in runs[1]] == want


def test_names_sizes_and_tag_rules():
    p = C.c_size_t(0)
    for blk, name, ies, oes in ((rr.ComplexToMag2(), "ComplexToMag2", 8, 4), (rr.SinglePoleIirFilter(0.1), "SinglePoleIirFilter", 4, 4),
                                (rr.SinglePoleIirFilter(0.1, np.complex64), "SinglePoleIirFilter", 8, 8),
                                (rr.BurstDetector(0.1, 1e-3), "ComplexToMag2>SinglePoleIirFilter>BurstTagger", 8, 4)):
        assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == 1 and p.value == 1   # RR_TAGS_FORWARD, position for position
        assert blk.name == name
        assert rr.lib().rr_block_in_elem_size(blk._h) == ies and rr.lib().rr_block_out_elem_size(blk._h) == oes
        assert blk.eof(True) and not blk.eof(False)
    assert rr.lib().rr_abi_version() == 3


# ---- 13. device-resident: channelizer -> detector through DeviceStreams ------------------------------------------------------------------
def test_device_streams_behind_the_channelizer():
    z = burst_signal(20000, 3)
    taps = rr.low_pass_complex(48000.0, 8000.0, 4000.0).reshape(1, -1)
    alpha, thr = 0.1, 1e-3
    # host windows: everything the channelizer gives for the whole input, then ONE detector call
    chan, parts, pos = rr.Channelizer(taps, 1, 2), [], 0
    for _ in range(1000):
        st, c, p, need, y = chan.work(z[pos:], 512_000)
        parts.append(np.asarray(y).reshape(-1)); pos += c
        if c == 0 and p == 0:
            break
    mid = np.concatenate(parts)
    assert len(mid) > 4 * T
    det = make_det(alpha, thr)
    env = det.work(mid, len(mid))[4]
    hpos, hval = det.edges()
    assert len(hpos) >= 4
    # the same two blocks between device-resident streams
    s0, s1, s2 = rr.DeviceStream(np.complex64), rr.DeviceStream(np.complex64), rr.DeviceStream(np.float32)
    assert s0.push(z) == len(z)
    chan2, det2 = rr.Channelizer(taps, 1, 2), make_det(alpha, thr)
    for _ in range(1000):
        st, c, p, need = chan2.work_streams(s0, s1)
        if c == 0 and p == 0:
            break
    assert s1.readable() == len(mid)
    st, c, p, need = det2.work_streams(s1, s2)
    assert (st, c, p, need) == sync_rule(len(mid), s2.capacity)
    env2 = s2.pop()
    dpos, dval = det2.edges()
    assert bits(env2).tolist() == bits(env).tolist()
    assert np.array_equal(dpos, hpos) and np.array_equal(dval, hval)


# ---- 14. the C++ mirror ---------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_burst():
    exe = os.path.join(ROOT, "tests", "cpp", "test_burst_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_burst_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK")
