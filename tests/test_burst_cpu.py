"""CPU-only: the models the GPU tests of rr_complex_to_mag2_create / rr_single_pole_iir_create / rr_burst_detector_create rely on
(tests/burst_model.py) — the reference's own test vectors through them, the bound of the reference's f32 fold, the proof that
the burst signal of the GPU tests has no sample whose comparison the two arithmetics could decide differently — and the
public surface of the three blocks."""
import ctypes

import numpy as np
import pytest

import rustradio_amd as rr
from burst_model import (bound_gpu, bound_gpu_any, bound_ref, bound_terms_any, burst_signal, coefficients, edges, iir_ref_f32,
                         iir_truth, iir_truth_const, iir_truth_ld, ld_truth_error, mag2_f32, state_size)


def test_reference_tag_it_through_the_model():
    """burst_tagger.rs tag_it: trigger 0.1 x 80, 0.3 x 10, 0.2 x 10, threshold 0.25 -> (80, true), (90, false)"""
    trig = np.array([0.1] * 80 + [0.3] * 10 + [0.2] * 10, np.float32)
    pos, val = edges(trig, 0.25)
    assert list(zip(pos.tolist(), val.tolist())) == [(80, True), (90, False)]
    # the same split over two calls, the flag carried
    p1, v1 = edges(trig[:85], 0.25)
    p2, v2 = edges(trig[85:], 0.25, last=bool(trig[84] > 0.25))
    assert list(zip(p1.tolist(), v1.tolist())) == [(80, True)] and list(zip(p2.tolist(), v2.tolist())) == [(5, False)]


def _create(alpha):
    """rr_single_pole_iir_create(alpha, 4) -> 'ok' | the library's error.  Without a device a good alpha still fails, later."""
    h = rr.lib().rr_single_pole_iir_create(ctypes.c_float(alpha), 4)
    if h:
        rr.lib().rr_block_destroy(h)
        return "ok"
    return rr.last_error()


def test_reference_reject_bad_alpha():
    """single_pole_iir_filter.rs reject_bad_alpha: 0, 0.1 and 1 are accepted, -0.1 and 1.1 are not (NaN: not contained either)"""
    for good in (0.0, 0.1, 1.0):
        assert "alpha out of range" not in _create(good)
    for bad in (-0.1, 1.1, float("nan"), float("inf")):
        assert _create(bad) == "alpha out of range"
        with pytest.raises(ValueError, match="alpha out of range"):
            rr.SinglePoleIirFilter(bad)
        with pytest.raises(ValueError, match="alpha out of range"):
            rr.BurstDetector(bad, 0.5)
    with pytest.raises(ValueError, match="alpha out of range"):
        rr.SinglePoleIirFilter(-0.1, np.complex64)


def test_models_agree_on_small_cases():
    x = np.array([0.1, 0.2], np.float32)                                           # iir_ff
    y, prev = iir_ref_f32(x, 0.2)
    t, _ = iir_truth(x, 0.2)
    assert np.max(np.abs(y - t)) <= bound_ref(0.2, 0.2) and prev == y[-1]
    assert mag2_f32(np.array([3 + 4j, 0.25 + 0j], np.complex64)).tolist() == [25.0, 0.0625]
    a, b = coefficients(0.01)
    assert a == float(np.float32(0.01)) and b == float(np.float32(1.0) - np.float32(0.01))
    # alpha 1: the input; alpha 0: zero
    assert np.array_equal(iir_ref_f32(x, 1.0)[0], x) and np.array_equal(iir_truth(x, 1.0)[0], x.astype(np.float64))
    assert not iir_ref_f32(x, 0.0)[0].any() and not iir_truth(x, 0.0)[0].any()


def test_closed_form_agrees_with_the_fold():
    segs = [(0.25, 5000), (0.0, 1), (0.25, 70_000), (0.0, 124_999)]
    x = np.concatenate([np.full(l, v, np.float32) for v, l in segs])
    t, _ = iir_truth(x, 0.01)
    d = float(np.max(np.abs(iir_truth_const(segs, 0.01) - t)))
    print(f"closed form vs f64 fold, {len(x)} samples, alpha 0.01: {d:.3e} (X = 0.25)")
    assert d <= 2.0 ** -53 * 0.25 * 4.0 / 0.01                                     # the fold's own roundings, damped


_SIG = {}


def _burst(alpha):
    """(x, t, y_ref) on burst_signal(60000, 7), shared"""
    if "x" not in _SIG:
        _SIG["x"] = mag2_f32(burst_signal(60000, 7))
    if alpha not in _SIG:
        _SIG[alpha] = (iir_truth(_SIG["x"], alpha)[0], iir_ref_f32(_SIG["x"], alpha)[0])
    return (_SIG["x"],) + _SIG[alpha]


@pytest.mark.parametrize("alpha", [0.5, 0.1, 0.01, 0.001])
def test_reference_fold_is_within_its_bound(alpha):
    x, t, y = _burst(alpha)
    X = float(np.max(np.abs(x)))
    e = float(np.max(np.abs(y.astype(np.float64) - t)))
    print(f"alpha {alpha}: f32 fold vs truth {e:.3e} = {e / bound_ref(X, alpha):.2f} of bound_ref {bound_ref(X, alpha):.3e}")
    assert e <= bound_ref(X, alpha)


@pytest.mark.parametrize("alpha,nedges", [(0.5, 8), (0.1, 8), (0.01, 6)])
def test_no_sample_of_the_burst_signal_is_ambiguous(alpha, nedges):
    """A condition of the GPU test against the reference: no sample lies so close to the threshold that the reference's f32
    fold and the GPU's cast f64 scan could fall on different sides.  Then both give the same edges: 4 bursts rise and fall,
    except that at alpha 0.01 the 3-sample burst never reaches the threshold."""
    thr = 1e-3
    x, t, y = _burst(alpha)
    X = float(np.max(np.abs(x)))
    ambiguous = int(np.sum(np.abs(t - float(np.float32(thr))) <= bound_ref(X, alpha) + bound_gpu(t, X, alpha)))
    assert ambiguous == 0
    pr, vr = edges(y, thr)
    pm, vm = edges(t.astype(np.float32), thr)
    assert np.array_equal(pr, pm) and np.array_equal(vr, vm)
    assert len(pr) == nedges and vr.tolist() == [True, False] * (nedges // 2)


# ---- the bound for every alpha (bound_gpu_any) is satisfiable, not loose, and never looser than bound_gpu -------------------------
T = 2048
_ALPHAS_ANY = [0.3, 1e-3, 2.0 ** -12, 1e-5, 0.6 * 2.0 ** -24, 2.0 ** -26, 0.999, 1.0 - 2.0 ** -24]


def dc_noise(n, seed):
    """0.5 + U(-0.5, 0.5): the DC keeps |t| away from zero, so the cast term is what a result is held to"""
    return (0.5 + np.random.default_rng(seed).uniform(-0.5, 0.5, n)).astype(np.float32)


def emulate_tile_tree(x, alpha):
    """The shape of the GPU's tree in f64 on the CPU, with MORE roundings than the kernel (multiply and add rounded
    separately where it has one fma): 8 samples per thread folded from zero, a Hillis-Steele scan over the 256 threads of a
    tile with pw8[k] = b^(8k) (long double, rounded once), y_in = base pw8[thread] + prefix, the fold again from y_in, one
    cast; tile bases sequentially, base' = base b^T + the tile's response.  One call from a zero state -> float32 outputs."""
    a, b = coefficients(alpha)
    pw8 = np.power(np.longdouble(b), np.arange(257, dtype=np.float64).astype(np.longdouble) * 8).astype(np.float64)
    n = len(x)
    xs = np.zeros((n + T - 1) // T * T)
    xs[:n] = np.asarray(x, np.float32)
    out, base, k = np.empty(len(xs)), 0.0, np.arange(256)
    for t0 in range(0, len(xs), T):
        v = xs[t0:t0 + T].reshape(256, 8)
        r = np.zeros(256)
        for i in range(8):
            r = b * r + a * v[:, i]
        inc, off = r.copy(), 1
        while off < 256:
            u = np.concatenate([np.zeros(off), inc[:-off]])
            inc = np.where(k >= off, u * pw8[off] + inc, inc)
            off *= 2
        y = base * pw8[k] + np.concatenate([[0.0], inc[:-1]])
        for i in range(8):
            y = b * y + a * v[:, i]
            out[t0 + i:t0 + T:8] = y
        base = base * pw8[256] + inc[255]
    return out[:n].astype(np.float32)


def test_long_double_has_64_bits():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    x = dc_noise(500, 1)
    assert np.max(np.abs(iir_truth_ld(x, 0.1)[0].astype(np.float64) - iir_truth(x, 0.1)[0])) <= 2.0 ** -53 * 4.0 / 0.1
    assert float(iir_truth_ld(x, 0.1)[1]) == float(iir_truth_ld(x, 0.1)[0][-1])


@pytest.mark.parametrize("alpha", _ALPHAS_ANY, ids=lambda a: f"{a:.9g}")
def test_any_alpha_bound_is_satisfiable_and_not_loose(alpha):
    """a correct tree fits the bound at every alpha, and the bound is at f32-ulp level everywhere: the f64 term stays far
    below the cast term, and the worst sample uses most of the allowance"""
    x = dc_noise(3 * T + 17, 40)
    t = iir_truth_ld(x, alpha)[0]
    y = emulate_tile_tree(x, alpha)
    cast, f64 = bound_terms_any(t, x, alpha)
    d = np.abs(y.astype(np.longdouble) - t).astype(np.float64)
    allow = cast + f64 + ld_truth_error(x, alpha)
    worst, ratio = float(np.max(d / allow)), float(np.median(f64 / cast))
    print(f"alpha {alpha:.6g}: emulated tree uses {worst:.3f} of bound_gpu_any, f64 term / cast term {ratio:.2e}")
    assert np.all(d <= allow)
    assert worst > 0.9 and ratio < 1e-3
    assert float(np.median(ld_truth_error(x, alpha) / cast)) < 1e-6                # the truth's own error blurs nothing


@pytest.mark.parametrize("alpha", [0.01, 0.3, 0.999])
def test_any_alpha_bound_is_never_looser_than_bound_gpu(alpha):
    x = dc_noise(3 * T + 17, 41)
    t = iir_truth(x, alpha)[0]
    for calls in (1, 7, 10_000):
        assert np.all(bound_gpu_any(t, x, alpha, calls) <= bound_gpu(t, float(np.max(np.abs(x))), alpha) * (1 + 1e-6))


def test_any_alpha_bound_at_the_ends():
    x = dc_noise(100, 42)
    a0, a1 = bound_terms_any(np.zeros(100), x, 0.0), bound_terms_any(x, x, 1.0, calls=3)
    assert np.all(a0[0] == 2.0 ** -150) and not a0[1].any()                        # alpha 0: the state is 0, only the floor
    assert np.all(a1[1] <= 2.0 ** -53 * 68.0)                                      # alpha 1: b = 0, M = X, R = 64 + 4
    assert state_size(x, 2.0 ** -26)[-1] == float(np.max(x)) * 2.0 ** -26 * 100    # b == 1: a plain sum
    sub = np.full(4, 2.0 ** -149, np.float32)
    assert np.all(bound_gpu_any(iir_truth(sub, 0.5)[0], sub, 0.5) < 2.0 ** -149)   # a subnormal result: under one ulp


def test_public_surface():
    from rustradio_amd._lib import SYMBOLS
    L = rr.lib()
    for s in ("rr_complex_to_mag2_create", "rr_single_pole_iir_create", "rr_burst_detector_create", "rr_burst_edges"):
        assert s in SYMBOLS and hasattr(ctypes.CDLL(rr.LIB_PATH), s)
    assert L.rr_single_pole_iir_create.argtypes == [ctypes.c_float, ctypes.c_size_t]
    assert L.rr_burst_detector_create.argtypes == [ctypes.c_float, ctypes.c_float]
    assert callable(rr.ComplexToMag2) and callable(rr.SinglePoleIirFilter) and callable(rr.BurstDetector.edges)
    assert L.rr_abi_version() == 3
    total = ctypes.c_size_t(7)
    assert L.rr_burst_edges(None, None, None, 0, ctypes.byref(total)) == rr.ERR    # no handle: an error, never a crash
    import torch
    if not torch.cuda.is_available():            # no CPU fallback: constructing any of them needs a device
        for make in (rr.ComplexToMag2, lambda: rr.SinglePoleIirFilter(0.01), lambda: rr.SinglePoleIirFilter(0.01, np.complex64),
                     lambda: rr.BurstDetector(0.01, 1e-3)):
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
