"""Test-side statement of Wpcr (src/wpcr.rs:105-239), written as the reference's SEQUENTIAL code — the slicing iterator, the
truncated transform, find_best_bin's loop, the f32 phase accumulator — so that it shares nothing with the GPU kernels' sparse
transform and integer clock.  Test infrastructure only: the product never imports it.

  find_best_bin        wpcr.rs:217-239 on a magnitude vector, in that vector's own precision (f32 magnitudes: f32 threshold)
  best_bin_margin      the smallest gap of any comparison find_best_bin makes on the way to its answer
  process_one          Wpcr::process_one (wpcr.rs:130-197) with a float64 numpy.fft standing in for rustfft, the clock and the
                       accumulator loop in f32; `mid` as the GPU block takes it (the reference: 0.0)
  picks_exact          the drift-free clock of rr_wpcr on fractions.Fraction: which samples, how many symbols, the end phase
  bound_spectrum       the bound of include/rustradio_amd.h on |X_gpu[k] - X[k]|
  nrz_burst            a burst builder: NRZ at a non-integer number of samples per symbol, random start phase, smoothing, noise
  g3ruh_burst          one G3RUH-scrambled, NRZI-coded frame between HDLC flags, and the bits that were sent
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from bits_model import HDLC_FLAG, ax25ish_symbols, hdlc_stuff, nrzi_encode, scramble

F32 = np.float32
E_SINCOS = 2.0 ** -21      # sincospif: (cos, sin) as a vector, 2 ulp per component at 1.0
# a phasor of the transform is sincospif's, or (three bins in four) the f32 product of two of them: twice the error of one
# (pi 2^-23 from the rounding of its phase, and e_sincos) and 3 2^-24 for the product.  In the bound's shape:
E_PHASOR = np.pi * 2.0 ** -23 + 2 * E_SINCOS + 3 * 2.0 ** -24
DEPTH = 20                 # f32 roundings behind a sum: 15 in a group of 16 terms, the cast of the f64 sum, norm_sqr().sqrt()'s 4


def find_best_bin(mag):
    """wpcr.rs:217-239 -> bin or None.  `mag` is what :222 computes; f32 in, f32 arithmetic."""
    mag = np.asarray(mag)
    skip = 2                                                   # :219
    if len(mag) <= skip:                                       # :229 `?`: max_by of nothing
        return None
    c08 = F32(0.8) if mag.dtype == np.float32 else float(F32(0.8))
    thresh = mag[skip:].max() * c08                            # :225-230
    for n in range(skip, len(mag) - 1):                        # :233 zip(mag, mag.skip(1)).enumerate().skip(skip)
        if mag[n] > thresh and mag[n] > mag[n + 1]:            # :234
            return n
    return None


def best_bin_margin(mag):
    """-> (bin or None, the smallest |a - b| of every comparison `a > b` find_best_bin evaluates before it returns)"""
    mag = np.asarray(mag, np.float64)
    if len(mag) <= 2:
        return None, np.inf
    thresh = mag[2:].max() * float(F32(0.8))
    gap = np.inf
    for n in range(2, len(mag) - 1):
        gap = min(gap, abs(mag[n] - thresh))
        if mag[n] > thresh:
            gap = min(gap, abs(mag[n] - mag[n + 1]))
            if mag[n] > mag[n + 1]:
                return n, gap
    return None, gap


def pulses(x, mid=0.0):
    """wpcr.rs:141-149: the 0/1 vector d, length n - 1"""
    with np.errstate(invalid="ignore"):
        s = (np.asarray(x, F32) > F32(mid)).astype(np.float64)
    return (s[:-1] - s[1:]) ** 2


def spectrum64(x, mid=0.0):
    """-> the float64 DFT of d, bins k < N / 2 (:153-156)"""
    d = pulses(x, mid)
    return np.fft.fft(d)[:len(d) // 2]


def accumulate_f32(x, p0, f):
    """wpcr.rs:180-186, the reference's loop in f32 -> (indices taken, end phase)"""
    phase, f = F32(p0), F32(f)
    one, taken = F32(1.0), []
    for i in range(len(x)):
        if phase >= one:
            phase = F32(phase - one)
            taken.append(i)
        phase = F32(phase + f)
    return np.array(taken, np.int64), phase


def clock_from(X, b, n):
    """:165-169 in f32 from a complex bin value -> (f, p0)"""
    f = F32(b) / F32(n)
    arg = F32(np.arctan2(F32(X.imag), F32(X.real)))
    t = F32(0.5) + arg / F32(2.0 * np.pi)
    p0 = t if t > F32(0.5) else F32(t + F32(1.0))
    return F32(f), F32(p0)


def process_one(x, mid=0.0, samp_rate=None):
    """Wpcr::process_one -> None or (symbols f32[], tags dict, bin, p0)"""
    x = np.asarray(x, F32)
    if len(x) < 4:                                             # :131-133
        return None
    X = spectrum64(x, mid)
    b = find_best_bin(np.abs(X))
    if b is None:
        return None
    f, p0 = clock_from(X[b], b, len(x))
    taken, phase = accumulate_f32(x, p0, f)
    tags = {"sps": f, "phase": phase}
    if samp_rate is not None:
        tags["frequency"] = F32(f * F32(samp_rate))            # :192
    return (x[taken] - F32(mid)).astype(F32), tags, b, p0


def fl32(q: Fraction):
    """the f32 nearest to a non-negative rational, ties to even"""
    if q == 0:
        return F32(0.0)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scaled = q / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    return F32(float(m) * 2.0 ** (e - 23))


def picks_exact(p0, f, n):
    """P(i) = p0 + i f in exact arithmetic on the two f32 values: sample i is taken iff floor(P(i)) > floor(P(i - 1)) (sample 0
    iff p0 >= 1) -> (indices taken, nsyms = floor(P(n - 1)), fl32(P(n) - nsyms))"""
    P0, Fq = Fraction(float(p0)), Fraction(float(f))
    D = max(P0.denominator, Fq.denominator)                    # powers of two
    A, B = int(P0 * D), int(Fq * D)
    assert Fraction(A, D) == P0 and Fraction(B, D) == Fq
    if n == 0:
        return np.zeros(0, np.int64), 0, fl32(P0)
    if A + n * B < 2 ** 62:
        fl = (A + np.arange(n, dtype=np.int64) * B) // D
    else:
        fl = np.array([(A + i * B) // D for i in range(n)], dtype=object)
    prev = np.concatenate([[0], fl[:-1]])
    taken = np.nonzero(fl > prev)[0].astype(np.int64)
    nsyms = int(fl[-1])
    assert len(taken) == nsyms and np.array_equal(np.asarray(fl[taken], np.int64) - 1, np.arange(nsyms))
    return taken, nsyms, fl32(P0 + n * Fq - nsyms)


def near_integer(p0, f, i):
    """|P(i) - nearest integer| for sample indices i (P(-1) for i = -1), in float64 (far more than the 2^-24 it is compared to)"""
    P = float(p0) + np.asarray(i, np.float64) * float(f)
    return np.abs(P - np.rint(P))


def bound_spectrum(C, e_sincos=E_PHASOR, depth=DEPTH):
    """|X_gpu[k] - X[k]| <= C (pi 2^-23 + e_sincos) + depth 2^-24 C"""
    return C * (np.pi * 2.0 ** -23 + e_sincos) + depth * 2.0 ** -24 * C


# the builder seeds the GPU tests use: tests/test_wpcr_cpu.py holds their decisive margin to 0.01 C (seeds 3 and 24 of the first
# 26 sit closer to a tie between two bins than that)
GPU_SEEDS = [s for s in range(26) if s not in (3, 24)]


def planted_offset(bits, tx, skip=2, search=range(12, 23)):
    """where the sent bits sit in a decoded stream (the scrambler delays by 17; the clock may gain or lose a symbol at the
    burst's edge): the offset d with bits[d + skip : d + len(tx)] == tx[skip:], or None"""
    bits, tx = np.asarray(bits, np.uint8), np.asarray(tx, np.uint8)
    for d in search:
        if d + len(tx) <= len(bits) and np.array_equal(bits[d + skip:d + len(tx)], tx[skip:]):
            return d
    return None


def upsample_nrz(levels, sps, rng, smooth=3, noise=0.05):
    """levels (+-1 per symbol) held for `sps` samples each from a random start phase, a moving average of `smooth` samples
    over it, Gaussian noise on top -> f32 burst"""
    levels = np.asarray(levels, np.float64)
    ph = rng.uniform(0.0, 1.0)
    n = int(np.floor((len(levels) - ph) * sps))
    idx = np.floor(np.arange(n) / sps + ph).astype(np.int64)
    x = levels[np.minimum(idx, len(levels) - 1)]
    if smooth > 1:
        x = np.convolve(x, np.ones(smooth) / smooth, mode="same")
    return (x + rng.normal(0.0, noise, n)).astype(F32)


def nrz_burst(seed, sps=None, n_frames=1):
    """an AX.25-like transmission (bits_model.ax25ish_symbols: flags, stuffed payload, NRZI, G3RUH, noise stretches) as an NRZ
    burst at `sps` samples per symbol (default: a seeded draw from [4.1, 9.7]) -> f32[]"""
    rng = np.random.default_rng(1000 + seed)
    soft, _ = ax25ish_symbols(n_frames, seed)
    if sps is None:
        sps = rng.uniform(4.1, 9.7)
    return upsample_nrz(np.where(soft > 0, 1.0, -1.0), sps, rng)


def g3ruh_burst(seed, sps=5.2083, nbits=300):
    """-> (burst f32[], tx bits): flag flag stuffed-payload flag, NRZI-encoded, G3RUH-scrambled by a transmitter that keys up
    afresh (17 more line symbols flush its register), as an NRZ burst with mild noise"""
    rng = np.random.default_rng(2000 + seed)
    tx = HDLC_FLAG + HDLC_FLAG + hdlc_stuff(rng.integers(0, 2, nbits).tolist()) + HDLC_FLAG
    line = scramble(nrzi_encode(tx) + [0] * 17)
    return upsample_nrz(2.0 * np.array(line, np.float64) - 1.0, sps, rng), np.array(tx, np.uint8)
