"""What the tests of rr.FskTx share (include/rustradio_amd.h).  Test infrastructure only; nothing here touches the GPU.

  Resampler / seq_chain   the reference's chains as they are written: RationalResampler's counter loop
                          (src/rational_resampler.rs:183-198), tx_model.vco_model twice, the Map / .re / MultiplyConst steps in f32
                          (examples/bell202.rs:166-183, g3ruh.rs:256-272)
  A, O, first, rep, src   the closed forms of the index maps, in Python integers
  truth1                  (sin, cos) of the exact stage-1 phase k1 (hi c1 + lo c0), long double, from the one-counts: no long sum
  truth2                  (sin, cos) of k2 * the running sum of a[src2(o)], long double, summed over audio runs with weights rep2
  audio_bound / out_bound the three bounds
  the packets, the framer's bits and the receive models of the loop-back tests
  the case files of tests/cpp/emu_fsk.cpp
"""
import functools
import math
import os
import struct
import subprocess

import numpy as np

import afsk_model as am
import frame_model as fm
import tx_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, AFSK = 0, 1
LD = np.longdouble
TWO_PI = LD(8) * np.arctan(LD(1))


def reduced(i, d):
    g = math.gcd(i, d)
    return i // g, d // g


# ---- closed forms (ratio reduced, Python integers) ------------------------------------------------------------------------------------
def made(n, i, d):
    """outputs after n inputs: ceil(n I / D)"""
    return -((-n * i) // d)


def first(k, i, d):
    """the first output of input k"""
    return made(k, i, d)


def rep(k, i, d):
    return first(k + 1, i, d) - first(k, i, d)


def src(m, i, d):
    """the input behind output m"""
    return (m * d) // i


def counts(splits, r1, r2):
    """[(n_audio, n_out)] of the pushes of `splits` bits from the start of the stream"""
    out, n0 = [], 0
    for n in splits:
        a0, a1 = made(n0, *r1), made(n0 + n, *r1)
        out.append((a1 - a0, made(a1, *r2) - made(a0, *r2)))
        n0 += n
    return out


# ---- the reference's chains, one sample after the other ---------------------------------------------------------------------------------
class Resampler:
    """rational_resampler.rs:183-198: counter += interp per input; while counter > 0: emit, counter -= deci.  (The reference
    reduces the ratio in new(); so does this.)"""

    def __init__(self, interp, deci):
        self.i, self.d = reduced(int(interp), int(deci))
        self.counter = 0

    def push(self, x):
        out = []
        for s in x:
            self.counter += self.i
            while self.counter > 0:
                out.append(s)
                self.counter -= self.d
        return out


def seq_chain(mode, bits, splits, i1, d1, lo, hi, k1, gain, i2, d2, k2=0.0):
    """-> (audio float32[] (AFSK; the gained Complex stream in DIRECT), out complex64[], [(n_audio, n_out) per push])"""
    rs1, rs2 = Resampler(i1, d1), Resampler(i2, d2)
    p1 = p2 = 0.0
    g = np.float32(gain)
    audio, out, cnt, at = [], [], [], 0
    for n in splits:
        b = [int(v) for v in bits[at:at + n]]
        at += n
        lv = np.array([hi if s > 0 else lo for s in rs1.push(b)], np.float32)           # Map
        v, p1 = tm.vco_model(lv, k1, p1)
        if mode == AFSK:
            a = (v.real.astype(np.float32) * g).astype(np.float32)                        # Map(.re) -> MultiplyConst
            audio.append(a)
            r = np.array(rs2.push(a.tolist()), np.float32)
            o, p2 = tm.vco_model(r, k2, p2)
        else:
            a = np.empty(len(v), np.complex64)                                            # MultiplyConst on Complex
            a.real = v.real.astype(np.float32) * g
            a.imag = v.imag.astype(np.float32) * g
            audio.append(a)
            o = np.array(rs2.push(a.tolist()), np.complex64)
        out.append(o)
        cnt.append((len(a), len(o)))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(audio, np.float32 if mode == AFSK else np.complex64), cat(out, np.complex64), cnt


# ---- truths ---------------------------------------------------------------------------------------------------------------------------
def _sincos(ph):
    ph = ph - TWO_PI * np.rint(ph / TWO_PI)
    return np.sin(ph), np.cos(ph)


def truth1(bits, n_audio, r1, lo, hi, k1):
    """(sin P1, cos P1)[m], m < n_audio, P1[m] = k1 (hi c1[m] + lo c0[m]) with c1 / c0 the one- / zero-samples up to and including
    m: the counts are exact integers and hi c1, lo c0 exact in long double (24 + 31 bits), so the phase is one sum and one
    product -> two long double arrays.  Own error: truth1_error."""
    b = (np.asarray(bits, np.uint8) != 0).astype(np.int64)
    m = np.arange(n_audio, dtype=np.int64)
    lv = b[(m * r1[1]) // r1[0]] if n_audio else np.zeros(0, np.int64)
    c1 = np.cumsum(lv)
    c0 = m + 1 - c1
    ph = LD(float(k1)) * (LD(np.float32(hi)) * c1.astype(LD) + LD(np.float32(lo)) * c0.astype(LD))
    return _sincos(ph)


def truth1_error(n_audio, d1):
    """per component: the sum, the product and the reduction's product and 2 pi each within 2^-64 of P <= n d1; long double sin"""
    return 4.0 * n_audio * d1 * 2.0 ** -64 + 2.0 ** -62


def _chunk(r2, d2):
    """terms of truth2 between two reductions of its carry: few enough that a chunk's partial sums stay below about 100"""
    r = -(-r2[0] // r2[1])
    return max(1, min(4096, int(100.0 / max(r * d2, 1e-300))))


def truth2(audio, r2, k2, sel=None):
    """(sin P2, cos P2)[o] (sel: at these outputs only), P2[o] = k2 * sum over o' <= o of a[src2(o')], from the start of the stream: a long-double sum over audio
    runs with weights rep2, the carry reduced modulo 2 pi every _chunk terms, j * (k2 a[m]) added inside a run.
    Own error: truth2_error."""
    a = np.asarray(audio, np.float32).astype(LD)
    na = len(a)
    chunk = _chunk(r2, abs(float(k2)) * float(np.max(np.abs(a))) if na else 0.0)
    m = np.arange(na + 1, dtype=np.int64)
    f = -((-m * r2[0]) // r2[1])                                   # first2(m)
    w = LD(float(k2)) * a * np.diff(f).astype(LD)
    base = np.zeros(na, LD)                                        # the phase in front of audio sample m
    carry = LD(0)
    for c0 in range(0, na, chunk):
        cs = np.cumsum(w[c0:c0 + chunk])
        base[c0:c0 + len(cs)] = carry + np.concatenate([np.zeros(1, LD), cs[:-1]])
        carry = carry + cs[-1]
        carry = carry - TWO_PI * np.rint(carry / TWO_PI)
    o = np.arange(int(f[-1]), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    mo = (o * r2[1]) // r2[0]
    j = o - f[mo] + 1
    ph = base[mo] + LD(float(k2)) * a[mo] * j.astype(LD)
    return _sincos(ph)


def truth2_error(n_audio, d2, r2):
    """per component.  With S = pi + (chunk + 1) rep d2, what no partial sum of a chunk exceeds: every weight and every addition
    of the chunk is within 2^-64 S of exact, 2 chunk S 2^-64 per chunk and carried on; each reduction of the carry costs S 2^-63
    (its product with a 2 pi that is itself within 2^-64 relative); the product inside the run, the last addition and the final
    reduction S 2^-62 together; long double sin and cos 2^-62."""
    chunk = _chunk(r2, d2)
    r = -(-r2[0] // r2[1])
    S = math.pi + (chunk + 1) * r * d2
    nchunks = -(-max(n_audio, 1) // chunk)
    return nchunks * (2.0 * chunk + 2.0) * S * 2.0 ** -64 + S * 2.0 ** -62 + 2.0 ** -62


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def audio_bound(m, gain, d1):
    """|a[m] - gain sin P1[m]| (and each DIRECT component), m counted from the stream's first audio sample"""
    return abs(gain) * (2.0 ** -24 + (np.asarray(m, np.float64) + 1.0) * (2.0 ** -48 + d1 * 2.0 ** -52))


def out_bound(o, d2):
    """each AFSK component against truth2 of the same push's audio: tx_model.bound_steps(o + 1, d2)"""
    return tm.bound_steps(np.asarray(o, np.float64) + 1.0, d2)


def d1_of(lo, hi, k1):
    return max(abs(k1 * float(np.float32(hi))), abs(k1 * float(np.float32(lo))))


def used_audio(got, bits, r1, lo, hi, k1, gain):
    """-> (largest |got - gain sin P1| / bound, the truth's own error / the smallest bound)"""
    got = np.asarray(got, np.float32)
    if len(got) == 0:
        return 0.0, 0.0
    sn, _ = truth1(bits, len(got), r1, lo, hi, k1)
    d1 = d1_of(lo, hi, k1)
    b = audio_bound(np.arange(len(got)), gain, d1)
    err = np.abs(got.astype(LD) - LD(np.float32(gain)) * sn).astype(np.float64)
    return float(np.max(err / b)), abs(gain) * truth1_error(len(got), d1) / float(b[0])


def used_direct(got, n_audio, bits, r1, r2, lo, hi, k1, gain, sel=None):
    """DIRECT: got = out, or out[sel] -> as used_audio"""
    got = np.asarray(got, np.complex64)
    if len(got) == 0:
        return 0.0, 0.0
    sn, cs = truth1(bits, n_audio, r1, lo, hi, k1)
    o = np.arange(len(got), dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    m = (o * r2[1]) // r2[0]
    d1 = d1_of(lo, hi, k1)
    b = audio_bound(m, gain, d1)
    g = LD(np.float32(gain))
    err = np.maximum(np.abs(got.real.astype(LD) - g * sn[m]), np.abs(got.imag.astype(LD) - g * cs[m])).astype(np.float64)
    return float(np.max(err / b)), abs(gain) * truth1_error(n_audio, d1) / float(b[0])


def used_out(got, audio, r2, k2, sel=None):
    """AFSK: `audio` is what the same pushes wrote; got = out, or out[sel] -> (largest error / bound, the truth's own error / the
    smallest bound)"""
    got = np.asarray(got, np.complex64)
    if len(got) == 0:
        return 0.0, 0.0
    sn, cs = truth2(audio, r2, k2, sel)
    assert len(sn) == len(got), (len(sn), len(got))
    d2 = abs(k2) * float(np.max(np.abs(audio)))
    b = out_bound(np.arange(len(got)) if sel is None else np.asarray(sel, np.int64), d2)
    err = np.maximum(np.abs(got.real.astype(LD) - sn), np.abs(got.imag.astype(LD) - cs)).astype(np.float64)
    return float(np.max(err / b)), truth2_error(len(audio), d2, r2) / float(b[0])


def patterns(n, seed):
    """name -> uint8[n]: random (with bytes other than 1 standing for a one), all-0, all-1, alternating"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2, n, dtype=np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return {"random": r, "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8), "alt": (np.arange(n) & 1).astype(np.uint8)}


def splits(rng, n, k):
    """k random cut points of n bits, with pushes of 0 and 1 bits put in"""
    at = np.sort(rng.integers(0, n + 1, k))
    lens = np.diff(np.concatenate([[0], at, [n]])).tolist()
    i = int(np.argmax(lens))
    if lens[i] > 2:
        lens[i:i + 1] = [1, 0, lens[i] - 1]
    return [int(v) for v in lens]


# ---- the loop-backs (afsk_model's receive parameters: 12 kS/s, 10 samples per symbol, SYNC_PRM, 289 taps) ----------------------------
LOOP_TX = dict(i1=10, d1=1, lo=1200.0, hi=2200.0, k1=2.0 * math.pi / 12000.0, gain=0.5, i2=4, d2=1, k2=2.0 * math.pi * 5000.0 / 48000.0)
LOOP_FLAGS = fm.FCS | fm.NRZI


def loop_packets():
    rng = np.random.default_rng(2202)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (12, 19, 33, 26, 40)]


@functools.lru_cache(maxsize=None)
def loop_bits():
    """rr_hdlc_framer(FCS | NRZI) over the packets, on the CPU (frame_model.FramerSeq) -> uint8[]"""
    out, _ = fm.FramerSeq(LOOP_FLAGS).push(loop_packets())
    out.setflags(write=False)
    return out


def loop_receive_model(soft):
    """SymbolSync -> HdlcReceiver(nrzi) on the models over one row of soft samples -> ([payload], stats)"""
    run = am.chain_model([np.asarray(soft, np.float32)], [len(soft)])
    return [f[1] for f in run[0]["frames"][0]], run[0]["stats"][0]


def demod_f64(audio):
    """rr.AfskDemod(1, 65, taps12k, 1.0, OFFSET) in float64 -> float32 soft samples"""
    return am.chain_f64(audio, am.hilbert(am.HIL), am.GAIN, am.taps12k(), am.OFFSET)["out"].astype(np.float32)


# ---- tests/cpp/emu_fsk.cpp ---------------------------------------------------------------------------------------------------------------
def build_cpp(name, exe, flags):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "rustradio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", name), "-o", exe], check=True)


def run_emu(exe, tmp, cases, tag="emu"):
    """cases: [(mode, bits, splits, i1, d1, lo, hi, k1, gain, i2, d2, k2)] -> per case (audio f32[], out c64[], [(na, no) per push])"""
    cf, rf = os.path.join(tmp, tag + "_cases.bin"), os.path.join(tmp, tag + "_results.bin")
    with open(cf, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for mode, bits, sp, i1, d1, lo, hi, k1, gain, i2, d2, k2 in cases:
            bits = np.ascontiguousarray(bits, np.uint8)
            assert sum(sp) == len(bits)
            f.write(struct.pack("<iqqffdfqqd", mode, i1, d1, lo, hi, k1, gain, i2, d2, k2))
            f.write(struct.pack("<i", len(sp)) + np.asarray(sp, np.int64).tobytes() + bits.tobytes())
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fsk core ok" in r.stdout, r.stdout + r.stderr
    buf, at, out = open(rf, "rb").read(), 0, []
    for case in cases:
        cnt = []
        for _ in case[2]:
            cnt.append(struct.unpack_from("<qq", buf, at))
            at += 16
        na, no = sum(c[0] for c in cnt), sum(c[1] for c in cnt)
        nau = na if case[0] == AFSK else 0
        audio = np.frombuffer(buf, np.float32, nau, at).copy(); at += 4 * nau
        o = np.frombuffer(buf, np.complex64, no, at).copy(); at += 8 * no
        out.append((audio, o, [tuple(int(v) for v in c) for c in cnt]))
    assert at == len(buf)
    return out
