"""Test-side statements of ComplexToMag2 (src/complex_to_mag2.rs:8-21), SinglePoleIirFilter (src/single_pole_iir_filter.rs:
11-93) and the comparison of BurstTagger (src/burst_tagger.rs:68-85).  Test infrastructure only: the product never imports
it, and none of the three is in the oracle.

  mag2_f32         re * re + im * im with three f32 roundings: what ComplexToMag2 IS
  iir_ref_f32      the reference's recurrence restated, a sequential f32 fold: what SinglePoleIirFilter IS there
  iir_truth        the recurrence on the widened coefficients in Python floats (f64): what the GPU block is judged against
  iir_truth_const  the closed form for piecewise-constant input, long double: the truth of the long cases
  iir_truth_ld     the recurrence in long double: the truth where an f64 fold's own roundings are not damped (tiny alpha)
  bound_gpu        how far the GPU's f32 output may be from the truth; bound_ref: how far the reference's f32 fold may be
  bound_gpu_any    the same for every alpha in [0, 1]: the f64 term follows the size of the state, not 1 / alpha
  edges            where BurstTagger pushes its tags
  burst_signal     noise with bursts, the input of examples/burst_saver.rs in miniature
"""
from __future__ import annotations

import numpy as np

BURSTS_60000 = [(5000, 7000), (20000, 3), (30000, 12000), (50000, 9000)]      # (start, length)


def coefficients(alpha):
    """the reference's two f32 fields (single_pole_iir_filter.rs:42-43), widened to f64: a = alpha, b = fl32(1 - alpha)"""
    a = np.float32(alpha)
    b = np.float32(np.float32(1.0) - a)
    return float(a), float(b)


def mag2_f32(z):
    z = np.asarray(z, np.complex64)
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((re * re).astype(np.float32) + (im * im).astype(np.float32)).astype(np.float32)


def iir_ref_f32(x, alpha, prev=0.0):
    """y = x * alpha + prev * one_minus_alpha in f32, three roundings per sample -> (float32 outputs, final prev)"""
    x = np.asarray(x, np.float32)
    a = np.float32(alpha)
    b = np.float32(np.float32(1.0) - a)
    out = np.empty(len(x), np.float32)
    prev = np.float32(prev)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(len(x)):
            prev = np.float32(np.float32(x[i] * a) + np.float32(prev * b))
            out[i] = prev
    return out, prev


def iir_truth(x, alpha, prev=0.0):
    """t[n] = a x[n] + b t[n-1], sequential, Python floats -> (float64 array, final t)"""
    a, b = coefficients(alpha)
    out = np.empty(len(x), np.float64)
    t = float(prev)
    for i, v in enumerate(np.asarray(x, np.float32).astype(np.float64).tolist()):
        t = a * v + b * t
        out[i] = t
    return out, t


def iir_truth_ld(x, alpha, prev=0.0):
    """iir_truth in np.longdouble (64 bits of mantissa where tests/test_burst_cpu.py asserts it) -> (longdouble array, final
    t).  Its own error is at most N 2^-62 M at the N-th sample (two roundings of 2^-64 M per step, undamped; M as in
    bound_terms_any): ld_truth_error, which the tests add to their allowance in the open."""
    ld = np.longdouble
    a, b = coefficients(alpha)
    a, b = ld(a), ld(b)
    out = np.empty(len(x), ld)
    t = ld(prev)
    for i, v in enumerate(np.asarray(x, np.float32).astype(ld)):
        t = a * v + b * t
        out[i] = t
    return out, t


def iir_truth_const(segments, alpha, prev=0.0):
    """segments = [(value, length)]: t = c' + (t_prev - c') b^(m+1) at the m-th sample of a segment, c' = a x / (1 - b),
    in long double -> float64 array.  Needs b < 1 (alpha > 0)."""
    ld = np.longdouble
    a, b = coefficients(alpha)
    a, b = ld(a), ld(b)
    out, t = [], ld(prev)
    for value, length in segments:
        c = a * ld(float(np.float32(value))) / (ld(1) - b)
        m = np.arange(1, length + 1, dtype=np.float64).astype(ld)
        seg = c + (t - c) * np.power(b, m)
        out.append(seg.astype(np.float64))
        t = seg[-1]
    return np.concatenate(out)


def edges(y, thr, last=False):
    """positions where cur = (y > thr) differs from the previous cur (`last` before sample 0) -> (uint64 pos, bool val)"""
    with np.errstate(invalid="ignore"):
        cur = np.asarray(y) > np.float32(thr)
    prev = np.concatenate([[bool(last)], cur[:-1]])
    pos = np.flatnonzero(cur != prev)
    return pos.astype(np.uint64), cur[pos]


def bound_gpu(t, X, alpha):
    """|out - t| allowed to the GPU block: the final cast to f32 (half an ulp, up to 2^-24 relative) and one f64 rounding of
    magnitude 2^-53 X per combination on a sample's path through the scan (at most 64), plus what is inherited through the
    carried prefix, damped by b per sample (the 1 / alpha)"""
    return 2.0 ** -24 * np.abs(t) + 2.0 ** -53 * X * (64.0 + 4.0 / alpha)


def state_size(x, alpha):
    """M[n]: what the state and every zero-state response on the way to sample n (N = n + 1 samples into the stream) are
    bounded by, as the sum of the absolute terms a |x[i]| b^(n-i): X min(a / (1 - b), a N), X = max |x| so far"""
    a, b = coefficients(alpha)
    x = np.abs(np.asarray(x, np.float32).astype(np.float64))
    X = np.maximum.accumulate(x) if len(x) else x
    grow = a * np.arange(1, len(x) + 1, dtype=np.float64)
    return X * (grow if b == 1.0 else np.minimum(a / (1.0 - b), grow))


def bound_terms_any(t, x, alpha, calls=1):
    """-> (cast term, f64 term) of bound_gpu_any.  The cast: half an ulp of the f32 delivered, 2^-24 |t| for a normal result
    and 2^-150 for a subnormal one.  The f64 term: 2^-53 M R, M = state_size and R the count of relative perturbations of
    2^-53 that reach a sample undamped: 64 + 4 / (1 - b) for any number of calls, as in bound_gpu, or 72 per
    moving call (43 roundings and 27 table entries on the longest path through one window), whichever is less.  `calls`: the
    moving calls so far, a call longer than one scan chunk (4096 tiles) counting once per chunk."""
    a, b = coefficients(alpha)
    t = np.abs(np.asarray(t).astype(np.float64))
    R = 72.0 * calls if b == 1.0 else min(64.0 + 4.0 / (1.0 - b), 72.0 * calls)
    return np.maximum(2.0 ** -24 * t, 2.0 ** -150), 2.0 ** -53 * state_size(x, alpha) * R


def bound_gpu_any(t, x, alpha, calls=1):
    """|out - t| allowed to the GPU block for every alpha in [0, 1] and results down to the f32 subnormals; never looser than
    bound_gpu where that one is valid (tests/test_burst_cpu.py)"""
    cast, f64 = bound_terms_any(t, x, alpha, calls)
    return cast + f64


def ld_truth_error(x, alpha):
    """iir_truth_ld's own distance from the exact recurrence: N 2^-62 M"""
    return np.arange(1, len(x) + 1, dtype=np.float64) * 2.0 ** -62 * state_size(x, alpha)


def bound_ref(X, alpha):
    """|y_ref - t| of the reference's f32 fold: three roundings of at most 2^-24 X per step, damped geometrically"""
    return 2.01 * 2.0 ** -24 * X / alpha


def burst_spans(n):
    return [(s * n // 60000, max(1, l * n // 60000) if l > 3 else l) for s, l in BURSTS_60000]


def burst_signal(n, seed):
    """complex Gaussian noise, sigma 0.003 per component, plus 0.1 e^(j 0.3 n) during the bursts (BURSTS_60000 scaled to n)"""
    rng = np.random.default_rng(seed)
    z = 0.003 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    k = np.arange(n)
    for s, l in burst_spans(n):
        z[s:s + l] += 0.1 * np.exp(1j * 0.3 * k[s:s + l])
    return z.astype(np.complex64)
