"""Test-side statements of Vco (src/vco.rs:9-37) and of RationalResampler -> Vco (examples/fm_tx.rs:84-91).  Test
infrastructure only: the product never imports it, and Vco is not in the oracle.

  vco_model   the reference's recurrence in Python floats (f64), sample by sample: what the block IS
  vco_truth   the same phase with no wrap rule and no tiles, in long double: what the block MEANS
  bound(n)    how far either may be from the other, per component, after n samples

For inputs on a dyadic grid (a = q / 2^g, q integer) the running sum is an integer, so the truth needs no long sum at all:
  vco_truth_grid   sin / cos of k * cumsum(q) / 2^g, exact up to ONE long-double product: the truth of the long cases, where
                   vco_truth's cumsum carries an error of its own (8.5e-7 on 8.4 M DC samples, 14 times bound(n))
  bound_steps      bound(n) widened for steps |k a| beyond 2 pi
  vco_step_model   the KERNEL's rule for such steps (whole turns removed from the step), sequential f64: CPU-only evidence
                   that bound_steps can be met
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

MX = 2.0 * math.pi                    # vco.rs: 2.0 * f64::consts::PI


def vco_model(a, k, phase=0.0):
    """phase += k * f64(a); one wrap by MX when it leaves [-MX, MX]; Complex(sin as f32, cos as f32)
    -> (complex64 outputs, final phase).  NaN compares false, Inf - MX = Inf, sin(Inf) = NaN: nothing special-cased."""
    a = np.asarray(a, np.float32)
    k = float(k)
    re = np.empty(len(a), np.float64)
    im = np.empty(len(a), np.float64)
    nan = float("nan")
    for i, s in enumerate(a.astype(np.float64).tolist()):
        phase += k * s
        if phase > MX:
            phase -= MX
        if phase < -MX:
            phase += MX
        if math.isfinite(phase):
            re[i] = math.sin(phase); im[i] = math.cos(phase)
        else:                         # math.sin(inf) raises where the reference's f64::sin returns NaN
            re[i] = nan; im[i] = nan
    out = np.empty(len(a), np.complex64)
    out.real = re.astype(np.float32)
    out.imag = im.astype(np.float32)
    return out, phase


def vco_truth(a, k):
    """(sin, cos) of k * cumsum(a) reduced mod 2 pi, everything in long double -> complex long double (re = sin)"""
    ld = np.longdouble
    ph = np.cumsum(ld(k) * np.asarray(a, np.float32).astype(ld))
    two_pi = ld(8) * np.arctan(ld(1))            # pi to long double precision (np.pi is the f64 value)
    ph = ph - two_pi * np.floor(ph / two_pi)
    return np.sin(ph) + 1j * np.cos(ph)


def bound(n):
    """absolute, per component, for |k a| <= 2 pi: 2^-25 is half an f32 ulp below 1 (the one rounding of the final cast);
    each of the n f64 additions of the phase contributes at most 2^-53 * 4 pi < 2^-49, doubled for the tile-level terms
    of a scan.  Derived, not measured."""
    return 2.0 ** -25 + n * 2.0 ** -48


GRID_G = 12                           # a = q / 2^12 with |q| <= 2^12: every a is an exact f32 in [-1, 1]


def grid_signal(q, g=GRID_G):
    """the f32 samples q / 2^g of integer q (exact: |q| <= 2^g <= 2^24)"""
    q = np.asarray(q, np.int64)
    assert g <= 24 and (len(q) == 0 or int(np.max(np.abs(q))) <= 1 << g)
    return (q.astype(np.float64) / float(1 << g)).astype(np.float32)


def grid_noise(n, seed, g=GRID_G):
    """uniform integer q in [-2^g, 2^g] -> (q, the f32 samples q / 2^g)"""
    q = np.random.default_rng(seed).integers(-(1 << g), (1 << g) + 1, n, dtype=np.int64)
    return q, grid_signal(q, g)


def truth_grid_error(n, k, g=GRID_G, qmax=None):
    """What vco_truth_grid itself may be off by, per component, anywhere in n samples of |q| <= qmax (default 2^g).
    With P = |k| n qmax / 2^g >= |k S| / 2^g, the largest phase before reduction:
      P 2^-64     the one product k * S in long double (64-bit significand; k and S enter exactly, the division by 2^g is exact)
      P 2^-64     the product two_pi * rint(.) of the reduction (their difference is then exact)
      P 2^-64     the long-double 2 pi is within half an ulp (2^-62) of 2 pi, times P / (2 pi) turns: P 2^-64.65
      2^-52       the reduced phase, in [-pi, pi], rounded to f64 (half an ulp of 2..4)
      2^-52       f64 sin / cos (glibc: under one ulp, and no value exceeds 1)
    The GPU tests assert that this is at most 1 % of the bound they judge with."""
    qmax = (1 << g) if qmax is None else qmax
    P = abs(float(k)) * n * qmax / float(1 << g)
    return 3.0 * P * 2.0 ** -64 + 2.0 ** -52 + 2.0 ** -52


def vco_truth_grid(q, g, k):
    """(sin, cos) of k * cumsum(q) / 2^g -> complex128 (re = sin).  cumsum(q) is exact in int64, so the phase is ONE long-double
    product, reduced modulo a long-double 2 pi; sin and cos are taken in f64 after the reduction.  Own error: truth_grid_error."""
    ld = np.longdouble
    q = np.asarray(q, np.int64)
    assert len(q) == 0 or len(q) * int(np.max(np.abs(q))) < 1 << 62
    S = np.cumsum(q)
    ph = ld(float(k)) * S.astype(ld) / ld(1 << g)
    two_pi = ld(8) * np.arctan(ld(1))
    ph -= two_pi * np.rint(ph / two_pi)                  # (rint: numpy's floor on long double is ten times slower)
    ph = ph.astype(np.float64)
    return np.sin(ph) + 1j * np.cos(ph)


def fm_tx_truth_grid(q, g, interp, deci, k, n_out):
    """vco_truth_grid over the resampled stream q[(m deci) // interp], m < n_out"""
    idx = (np.arange(n_out, dtype=np.int64) * int(deci)) // int(interp)
    return vco_truth_grid(np.asarray(q, np.int64)[idx], g, k)


def bound_steps(n, dmax):
    """bound(n) for steps of any size, dmax = max |k a|:  2^-25 + n (2^-48 + dmax 2^-52).
    The first two terms are bound(n): the final f32 cast and the additions of a phase kept inside [-2 MX, 2 MX].  What a large
    step adds, per sample:
      dmax 2^-53   the product k * a, rounded once to f64 (half an ulp of a value <= dmax)
      dmax 2^-54   every whole turn taken out of the step is f64(2 pi), which is 2.45e-16 < 2^-51.8 away from 2 pi, and there
                   are at most dmax / (2 pi) of them: dmax 2^-51.8 / 2^2.65 < dmax 2^-54
    together 0.75 dmax 2^-52 < dmax 2^-52.  (For dmax <= 2 pi the extra term is below n 2^-49: the product's rounding, which
    bound(n) already holds inside its 2^-48.)  Derived, not measured."""
    return 2.0 ** -25 + n * (2.0 ** -48 + dmax * 2.0 ** -52)


def vco_step_model(a, k, phase=0.0):
    """The kernel's rule (kernels_tx.hip vco_step / vco_wrap), NOT the reference's, one sample after the other in f64:
    d = k * a; beyond 2 MX, d = fma(-MX, trunc(d * (1 / MX)), d); wrap d; phase = wrap(phase + d); (sin, cos) as f32
    -> (complex64 outputs, final phase).  The fma is formed exactly in rationals and rounded once (no math.fma before 3.13).
    CPU only, finite input only: it shows that bound_steps is attainable, no GPU test is judged by it."""
    def wrap(p):
        if p > MX:
            p -= MX
        if p < -MX:
            p += MX
        return p
    a = np.asarray(a, np.float32)
    k = float(k)
    FMX, inv = Fraction(MX), 1.0 / MX
    re = np.empty(len(a), np.float64)
    im = np.empty(len(a), np.float64)
    for i, s in enumerate(a.astype(np.float64).tolist()):
        d = k * s
        if abs(d) > 2.0 * MX:
            d = float(Fraction(d) - FMX * Fraction(float(math.trunc(d * inv))))
        phase = wrap(phase + wrap(d))
        re[i] = math.sin(phase); im[i] = math.cos(phase)
    out = np.empty(len(a), np.complex64)
    out.real = re.astype(np.float32)
    out.imag = im.astype(np.float32)
    return out, phase


def fm_tx_truth(x, interp, deci, k, n_out):
    """vco_truth over the resampled stream r[m] = x[(m deci) // interp], m < n_out (the ratio as given)"""
    idx = (np.arange(n_out, dtype=np.int64) * int(deci)) // int(interp)
    return vco_truth(np.asarray(x, np.float32)[idx], k)


def comp_err(got, truth):
    """largest per-component distance of complex64 outputs from a complex long double truth"""
    ld = np.longdouble
    g = np.asarray(got)
    if len(g) == 0:
        return 0.0
    return float(max(np.max(np.abs(g.real.astype(ld) - truth.real)), np.max(np.abs(g.imag.astype(ld) - truth.imag))))


def sync_rule(in_len, out_cap):
    """(status, consumed, produced, need) of a #[rustradio(sync)] block (rustradio_macros_code/src/lib.rs:458-515)"""
    WAIT_SRC, WAIT_DST = 1, 2
    if in_len == 0:
        return (WAIT_SRC, 0, 0, 1)
    if out_cap == 0:
        return (WAIT_DST, 0, 0, 1)
    n = min(in_len, out_cap)
    return (WAIT_SRC if n == in_len else WAIT_DST, n, n, 1)
