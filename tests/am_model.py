"""What the tests of rr.AmDemod share: the float64 form of the block's definition (include/rustradio_amd.h), the bound a device
or host result is held to against it, the cut and NaN-set helpers, the AM test signals, and the case files of
tests/cpp/emu_am.cpp.  Nothing here touches the GPU."""
import functools
import math
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def reduced(I, D):
    g = math.gcd(int(I), int(D))
    return int(I) // g, int(D) // g


def count(N, I, D):
    """O(N) = ceil(N I / D)"""
    I, D = reduced(I, D)
    return (int(N) * I + D - 1) // D


def picks(n_out, I, D):
    """p(o) = floor(o D / I), o < n_out -> int64[n_out]"""
    I, D = reduced(I, D)
    return (np.arange(n_out, dtype=np.int64) * D) // I


def mag64(x):
    """the exact magnitudes of Complex samples: the squares of f32 are exact in f64 -> float64 (one add, one sqrt)"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    return np.sqrt(re * re + im * im)


def mag32(x):
    """m of the definition: the f64 formula narrowed once -> float32"""
    return mag64(x).astype(np.float32)


def chain_f64(x, taps, I, D, scale):
    """the definition in float64 (exact m, exact sums) -> dict: out float64[ceil(N I / D)], absum (sum_j |taps[j]| m64[p - j] at
    every output), p"""
    m = mag64(x)
    t = np.asarray(taps, np.float64)
    N = len(m)
    p = picks(count(N, I, D), I, D)
    if N == 0:
        return {"out": np.zeros(0), "absum": np.zeros(0), "p": p}
    y = np.convolve(m, t)[:N]
    ab = np.convolve(m, np.abs(t))[:N]
    return {"out": float(scale) * y[p], "absum": ab[p], "p": p}


def bound(ref, L, scale):
    """B[o] = 1.01 (L + 2) 2^-24 |scale| sum_j |taps[j]| m64[p(o) - j]"""
    return 1.01 * (L + 2) * 2.0 ** -24 * abs(float(scale)) * ref["absum"]


def used(got, ref, L, scale, extra=0.0):
    """-> the largest |got - out| / (B + extra) (must be <= 1); got must be finite and of the definition's length"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref["out"].shape, (got.shape, ref["out"].shape)
    if len(got) == 0:
        return 0.0
    assert np.all(np.isfinite(got))
    b = bound(ref, L, scale) + extra
    assert np.all(b > 0)
    return float(np.max(np.abs(got - ref["out"]) / b))


def samples_for_outputs(k, I, D):
    """the smallest N with ceil(N I / D) >= k"""
    I, D = reduced(I, D)
    N = (int(k) * D) // I
    while count(N, I, D) < k:
        N += 1
    while N > 0 and count(N - 1, I, D) >= k:
        N -= 1
    return N


def nan_set(k, n_out, L, I, D):
    """outputs a NaN at x[k] makes NaN: p(o) - L + 1 <= k <= p(o) -> bool[n_out]"""
    p = picks(n_out, I, D)
    return (p - L + 1 <= k) & (k <= p)


def split_lens(rng, n, k):
    """k random cut points of n samples, with pushes of 0 and 1 samples put in"""
    at = np.sort(rng.integers(0, n + 1, k))
    lens = np.diff(np.concatenate([[0], at, [n]])).tolist()
    i = int(np.argmax(lens))
    if lens[i] > 2:                            # a 1-sample push and an empty one in front of the longest
        lens[i:i + 1] = [1, 0, lens[i] - 1]
    return [int(v) for v in lens]


# ---- signals -------------------------------------------------------------------------------------------------------------------------
def am_signal(n, seed=0, amp=1.0, wa=0.05, noise=1e-3):
    """a carrier A e^{j phi} with the envelope 1 + 0.5 cos(wa k + q), plus small noise -> complex64[n]: |x| stays within
    [0.5 A, 1.5 A] or so, and a low-pass of unit DC gain over it gives outputs near A, far from subnormal"""
    rng = np.random.default_rng(9000 + seed)
    k = np.arange(n)
    phi, q = rng.uniform(0, 2 * np.pi, 2)
    env = 1.0 + 0.5 * np.cos(wa * k + q)
    x = amp * env * np.exp(1j * (0.013 * k + phi))
    x = x + amp * noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def lp_taps(L, cutoff=0.1):
    """L taps of a plausible low-pass: a windowed sinc of the given cutoff (of fs) with unit DC gain (L == 1: the identity)"""
    if L == 1:
        return np.ones(1, np.float32)
    k = np.arange(L) - (L - 1) / 2.0
    t = np.sinc(2.0 * cutoff * k) * np.hamming(L)
    return (t / t.sum()).astype(np.float32)


def taps_for(L):
    """a cutoff that narrows with the filter, as a designer's would"""
    return lp_taps(L, min(0.1, 8.0 / L))


# the end-to-end signal: 3 AM stations in one AirSPY stream
E2E_FS, E2E_N, E2E_DECI = 1.0, 36000, 12
E2E_OFFSETS = (-0.25, 0.0, 0.25)              # of fs: multiples of the channel rate fs / 12, so each folds to DC
E2E_TONES = (0.0011, 0.0017, 0.0023)          # of fs
E2E_RF_TAPS, E2E_AUDIO_TAPS = 257, 129
E2E_AUDIO = (1, 5)                            # I : D behind the channelizer


def e2e_iq():
    """-> (uint32[n] AirSPY words, complex64[n] what AirspyDecode makes of them)"""
    k = np.arange(E2E_N)
    x = np.zeros(E2E_N, np.complex128)
    for f0, fa in zip(E2E_OFFSETS, E2E_TONES):
        x += 5.0 * (1.0 + 0.5 * np.cos(2 * np.pi * fa * k)) * np.exp(2j * np.pi * f0 * k)
    x += 0.02 * (np.random.default_rng(77).standard_normal(E2E_N) + 1j * np.random.default_rng(78).standard_normal(E2E_N))
    i16 = np.round(x.real * 1000.0).astype(np.int16)
    q16 = np.round(x.imag * 1000.0).astype(np.int16)
    words = (i16.astype(np.uint16).astype(np.uint32)) | (q16.astype(np.uint16).astype(np.uint32) << 16)
    dec = (i16.astype(np.float32) / np.float32(1000)) + 1j * (q16.astype(np.float32) / np.float32(1000))
    return words, dec.astype(np.complex64)


def e2e_rf_taps():
    """a 257-tap low-pass of cutoff 0.03 fs shifted to every station -> complex64[3, 257]"""
    t = lp_taps(E2E_RF_TAPS, 0.03).astype(np.float64)
    k = np.arange(E2E_RF_TAPS)
    return np.stack([t * np.exp(2j * np.pi * f0 * k) for f0 in E2E_OFFSETS]).astype(np.complex64)


def e2e_audio_taps():
    return lp_taps(E2E_AUDIO_TAPS, 0.04)


def e2e_model():
    """the float64 model of the whole path -> float64[3, n_audio]"""
    _, x = e2e_iq()
    rows = []
    for t in e2e_rf_taps():
        y = np.convolve(x.astype(np.complex128), t.astype(np.complex128))[:len(x)]
        ch = y[::E2E_DECI]
        rows.append(chain_f64(ch.astype(np.complex64), e2e_audio_taps(), *E2E_AUDIO, 1.0)["out"])
    return np.stack(rows)


def e2e_scores(audio):
    """audio [3, n] -> corr[c][s]: |correlation| of channel c's audio, mean removed, start-up dropped, with the best-fitting
    sinusoid of station s's tone"""
    audio = np.asarray(audio, np.float64)
    step = E2E_DECI * E2E_AUDIO[1] / E2E_AUDIO[0]
    skip = 40
    out = np.zeros((3, 3))
    for c in range(3):
        a = audio[c, skip:]
        a = a - a.mean()
        k = (np.arange(len(a)) + skip) * step
        for s, fa in enumerate(E2E_TONES):
            # the largest correlation with cos(w k + phase) over every phase: the share of a in the span of (cos, sin)
            B = np.stack([np.cos(2 * np.pi * fa * k), np.sin(2 * np.pi * fa * k)], axis=1)
            B = B - B.mean(axis=0)
            coef = np.linalg.lstsq(B, a, rcond=None)[0]
            out[c, s] = np.linalg.norm(B @ coef) / (np.linalg.norm(a) + 1e-300)
    return out


# ---- tests/cpp/emu_am.cpp ------------------------------------------------------------------------------------------------------------
def write_cases(path, cases):
    """cases: [(x complex64[nstreams, n], taps, I, D, scale, [push lengths])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for x, taps, I, D, scale, lens in cases:
            x = np.ascontiguousarray(x, np.complex64)
            assert x.ndim == 2 and sum(lens) == x.shape[1]
            f.write(struct.pack("<iiqqf", x.shape[0], len(taps), I, D, scale))
            f.write(np.asarray(taps, np.float32).tobytes())
            f.write(struct.pack("<i", len(lens)) + np.asarray(lens, np.int32).tobytes())
            at = 0
            for n in lens:
                f.write(np.ascontiguousarray(x[:, at:at + n]).tobytes())
                at += n


def read_results(path, cases):
    """-> per case [per push float32[nstreams, produced]]"""
    buf, at, out = open(path, "rb").read(), 0, []
    for x, _, _, _, _, lens in cases:
        pushes = []
        for _ in lens:
            k = struct.unpack_from("<i", buf, at)[0]
            at += 4
            pushes.append(np.frombuffer(buf, np.float32, x.shape[0] * k, at).reshape(x.shape[0], k).copy())
            at += 4 * x.shape[0] * k
        out.append(pushes)
    assert at == len(buf)
    return out


def build_emu(exe, flags=()):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "rustradio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "emu_am.cpp"), "-o", exe], check=True)


def run_emu(exe, tmp, cases, tag="emu"):
    cf, rf = os.path.join(tmp, tag + "_cases.bin"), os.path.join(tmp, tag + "_results.bin")
    write_cases(cf, cases)
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "am core ok" in r.stdout, r.stdout + r.stderr
    return read_results(rf, cases)


def emu_dims(exe, L, I, D):
    """-> (T, C): what rr_am_demod_dims says on a device, from the same am_geom"""
    r = subprocess.run([exe, "--dims", str(L), str(I), str(D)], capture_output=True, text=True, check=True)
    T, C, _, _ = (int(v) for v in r.stdout.split())
    return T, C


@functools.lru_cache(maxsize=None)
def plain_emu():
    """the emulator built without sanitizers (the GPU tests' host twin), once per process -> (exe, its directory)"""
    d = tempfile.mkdtemp(prefix="am_emu_")
    exe = os.path.join(d, "emu_am")
    build_emu(exe, ["-O2"])
    return exe, d


def twin(x, taps, I, D, scale, lens=None):
    """the host twin of am_host.hpp over the rows of x in pushes of `lens` (default: one) -> float32[nstreams, produced]"""
    x = np.ascontiguousarray(x, np.complex64)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    exe, d = plain_emu()
    res = run_emu(exe, d, [(x, taps, I, D, scale, lens or [x.shape[1]])], "twin")
    return np.concatenate(res[0], axis=1)
