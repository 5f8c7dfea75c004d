"""What the tests of rr.AfskDemod share: the float64 form of the block's definition (include/rustradio_amd.h), the bound a device
or host result is held to against it, the 16-stream Bell 202 signal of the end-to-end tests, the two-tone row of the shape tests,
and the case files of tests/cpp/emu_afsk.cpp.  Nothing here touches the GPU."""
import functools
import os
import struct
import subprocess

import numpy as np

import hdlc_model as hm
import hdlcrx_helpers as hx
import rustradio_amd as rr
import rx_chain_helpers as rc
import symsync_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


def hilbert(H, window=rr.WIN_HAMMING, parm=0.0):
    """hilbert_taps(make_window(window, H, parm)) -> float32[H] (the library's host-side designer; no device)"""
    return rr.hilbert_taps(rr.make_window(window, H, parm))


def analytic_f64(x, hil):
    """a[m] = (xp[m + H/2], sum_j hil[H-1-j] xp[m + j]), xp = H zeros ++ x, m = 0 .. T-1 -> complex128[T]"""
    x, hil = np.asarray(x, np.float64), np.asarray(hil, np.float64)
    H, T = len(hil), len(x)
    xp = np.concatenate([np.zeros(H), x])
    im = np.convolve(xp, hil)[H - 1:H - 1 + T]
    return xp[H // 2:H // 2 + T] + 1j * im


def chain_f64(x, hil, gain, taps, offset):
    """the definition in float64 -> dict: out float64[max(T - 1, 0)], y (before the offset), d, a"""
    a = analytic_f64(x, hil)
    d = gain * np.angle(a[1:] * np.conj(a[:-1])) if len(a) > 1 else np.zeros(0)
    y = np.convolve(d, np.asarray(taps, np.float64))[:len(d)] if len(d) else d
    return {"out": y + offset, "y": y, "d": d, "a": a}


def bound(ref, gain, taps):
    """per output i: sum_j |taps[j]| b[i - j] + 1e-5 max|y|, b = harness.angle_parity's per-sample bound (tol 1e-5) on the
    float64 analytic stream (times |gain|), max|y| taken before the offset"""
    if len(ref["d"]) == 0:
        return np.zeros(0)
    b = abs(gain) * rc.angle_bound(ref["a"], TOL)
    return np.convolve(b, np.abs(np.asarray(taps, np.float64)))[:len(b)] + TOL * float(np.max(np.abs(ref["y"])))


def used(got, ref, gain, taps):
    """-> the largest |got - out| / bound (must be <= 1); got must be finite and of the definition's length"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref["out"].shape, (got.shape, ref["out"].shape)
    if len(got) == 0:
        return 0.0
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref["out"]) / bound(ref, gain, taps)))


# ---- the 16-stream Bell 202 signal -------------------------------------------------------------------------------------------------
FS, BAUD, SPS, NSTREAMS, HIL = 12000.0, 1200.0, 10, 16, 65
MARK, SPACE = 1200.0, 2200.0
SYNC_PRM, MAX_SIZE = (10.0, 0.5, [0.1, 0.9]), 60
OFFSET = -1700.0 * 2.0 * np.pi / FS
GAIN = 1.0


def taps12k():
    return rr.low_pass(FS, 1100.0, 100.0)                     # 289 taps


def payloads(c):
    rng = np.random.default_rng(1200 + c)
    return [rng.integers(0, 256, 12 + 7 * (c % 5), dtype=np.uint8).tobytes() for _ in range(3)]


def levels(c):
    bits, k = hm.FLAG * 24, 2 + c % 3
    for p in payloads(c):
        bits = bits + hm.frame_bits(p, k, k)
    return hx.line_encode(bits + hm.FLAG * 6, nrzi=True)


@functools.lru_cache(maxsize=None)
def _waves():
    return [sm.hold(levels(c), SPS, ((5 * c) % 13 - 6) * 0.0007) for c in range(NSTREAMS)]


@functools.lru_cache(maxsize=None)
def samples():
    """-> (float32[16, n] read-only, [unpadded length of row c]): 2200 Hz for a positive level, 1200 Hz otherwise, phase-continuous,
    0.5 cos + 0.02 N(0, 1); the shorter rows go on in their last tone"""
    waves = _waves()
    n = max(len(w) for w in waves)
    rows = []
    for c, w in enumerate(waves):
        w = np.concatenate([w, np.full(n - len(w), w[-1], np.float32)])
        f = np.where(w > 0, SPACE, MARK)
        ph = 2.0 * np.pi * np.cumsum(f) / FS
        rows.append((0.5 * np.cos(ph) + 0.02 * np.random.default_rng(7 + c).standard_normal(n)).astype(np.float32))
    x = np.stack(rows)
    x.setflags(write=False)
    return x, [len(w) for w in waves]


@functools.lru_cache(maxsize=None)
def reference(c):
    """the float64 chain over the padded row c"""
    return chain_f64(samples()[0][c], hilbert(HIL), GAIN, taps12k(), OFFSET)


def cuts(n):
    return rc.ragged_cuts(n)


def chain_model(rows, soft_cuts):
    """SymbolSync(10.0, 0.5, [0.1, 0.9]) -> ModelReceiver(1, 60, nrzi) per row over pushes of soft samples (rx_chain_helpers)"""
    return rc.chain_model(rows, soft_cuts, SYNC_PRM, (1, MAX_SIZE), dict(nrzi=True))


def soft_cuts(sample_cuts):
    """outputs of each push of samples: one fewer for the first that holds any"""
    out, seen = [], 0
    for n in sample_cuts:
        out.append(n if seen else max(n - 1, 0))
        seen += n
    return out


# ---- the two-tone row of the shape tests ---------------------------------------------------------------------------------------------
def two_tone(n, seed=0):
    """0.6 cos(0.21 i + p) + 0.3 cos(0.47 i + q): |a| stays between 0.3 and 0.9 behind the Hilbert start-up -> float32[n]"""
    rng = np.random.default_rng(4000 + seed)
    i = np.arange(n)
    p, q = rng.uniform(0, 2 * np.pi, 2)
    return (0.6 * np.cos(0.21 * i + p) + 0.3 * np.cos(0.47 * i + q)).astype(np.float32)


def lp_taps(L, seed=0):
    """L taps of a plausible low-pass: a windowed sinc of cutoff 0.1 fs with unit DC gain (L == 1: the identity)"""
    if L == 1:
        return np.ones(1, np.float32)
    k = np.arange(L) - (L - 1) / 2.0
    t = np.sinc(0.2 * k) * np.hamming(L)
    return (t / t.sum()).astype(np.float32)


# ---- tests/cpp/emu_afsk.cpp ---------------------------------------------------------------------------------------------------------
def write_cases(path, cases):
    """cases: [(x float32[nstreams, n], hil, gain, taps, offset, [push lengths])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for x, hil, gain, taps, offset, lens in cases:
            x = np.ascontiguousarray(x, np.float32)
            assert x.ndim == 2 and sum(lens) == x.shape[1]
            f.write(struct.pack("<iiiff", x.shape[0], len(hil), len(taps), gain, offset))
            f.write(np.asarray(hil, np.float32).tobytes() + np.asarray(taps, np.float32).tobytes())
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


def build_emu(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "rustradio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "emu_afsk.cpp"), "-o", exe], check=True)


def run_emu(exe, tmp, cases, tag="emu"):
    cf, rf = os.path.join(tmp, tag + "_cases.bin"), os.path.join(tmp, tag + "_results.bin")
    write_cases(cf, cases)
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "afsk core ok" in r.stdout, r.stdout + r.stderr
    return read_results(rf, cases)
