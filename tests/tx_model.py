"""Test-side statements of Vco (src/vco.rs:9-37) and of RationalResampler -> Vco (examples/fm_tx.rs:84-91).  Test
infrastructure only: the product never imports it, and Vco is not in the oracle.

  vco_model   the reference's recurrence in Python floats (f64), sample by sample: what the block IS
  vco_truth   the same phase with no wrap rule and no tiles, in long double: what the block MEANS
  bound(n)    how far either may be from the other, per component, after n samples
"""
from __future__ import annotations

import math

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
