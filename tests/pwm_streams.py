"""What the PwmDecoder tests share: Pair (a handle and a PwmModel fed the same samples, every delivery compared exactly), the
run-length builders of clean 0/1 streams, and the generators of the streams that take the candidate table of k_pwm_walk past its
boundaries (tests/test_gpu_pwm_table.py on the device, tests/test_pwm_table_cpu.py on the model alone).  Nothing in here needs a
device until a Pair is made.

A generator returns a Case: the settings, the f32 samples, the words it sent and named cut points.  Everything is drawn from a
fixed seed, so both test files see the same streams."""
from collections import namedtuple

import numpy as np

import pwm_model as pm
import rustradio_amd as rr

TILE = 2048                                   # pwm_core.hpp's PWM_T; the GPU tests hold dims() to it, the CPU test the header
SHORT, LONG, FGAP, RGAP = 2, 5, 9, 20
POS = [0.5, SHORT, LONG, FGAP, RGAP]
BASE = (POS, dict(low_threshold=0.25, pulse_tolerance=1, max_frame_bits=16, max_distinct_frames=4))
BIT = SHORT + LONG                            # samples of one bit of word()

Case = namedtuple("Case", "pos kw x words cuts")


def settings(**kw):
    """BASE with other keyword settings"""
    return list(POS), dict(BASE[1], **kw)


def frames_of(result):
    return [(tuple(int(b) for b in bits), repeats, first) for bits, repeats, first in result]


class Pair:
    def __init__(self, pos, kw, dtype=np.float32):
        self.dev = rr.PwmDecoder(*pos, **kw, dtype=dtype)
        self.model = pm.PwmModel(*pos, **kw)
        self.pos, self.kw, self.dtype = pos, kw, np.dtype(dtype)

    def feed(self, x, via="push", z=None):
        """the next samples through both -> the frames delivered, asserted equal.  z: what the handle is given in place of x
        (the Complex samples whose power x is)"""
        x = np.ascontiguousarray(x, np.float32)
        d = x if z is None else np.ascontiguousarray(z, self.dtype)
        assert len(d) == len(x)
        want = self.model.push(x)
        if via == "push":
            got = frames_of(self.dev.push(d))
        else:
            import torch
            t = torch.from_numpy(d.view(np.float32)).cuda()
            self.dev.push_dev(t.data_ptr() if len(d) else 0, len(d))
            got = frames_of(self.dev.result())
        assert got == want, (len(x), len(got), len(want), got[:3], want[:3])
        return got

    def feed_cut(self, x, cuts, via="push", z=None):
        out, at = [], 0
        for c in list(cuts) + [len(x)]:
            out.append(self.feed(x[at:c], via, None if z is None else z[at:c]))
            at = c
        return out

    def flush(self):
        got, want = frames_of(self.dev.flush()), self.model.flush()
        assert got == want
        return got


def runs(*pairs):
    """(high, count) runs -> f32 samples, 1.0 and 0.0"""
    return np.concatenate([np.full(c, 1.0 if h else 0.0, np.float32) for h, c in pairs] or [np.zeros(0, np.float32)])


def word(bits, gap=FGAP, delimiter=False):
    """add_frame (src/pwm_decoder.rs:702-712) with the gap behind it"""
    r = []
    for b in bits:
        r += [(True, SHORT if b else LONG), (False, LONG if b else SHORT)]
    if delimiter:
        r.append((True, SHORT))
    r.append((False, gap))
    return r


def words_stream(words, last_gap=RGAP):
    """the words one behind the other, frame_gap between them and last_gap behind the last -> (samples, where each word begins,
    with the stream's length as the last entry)"""
    parts = [runs(*word(w, last_gap if i == len(words) - 1 else FGAP)) for i, w in enumerate(words)]
    return np.concatenate(parts), np.cumsum([0] + [len(p) for p in parts])


def distinct_words(rng, count, nbits):
    """count distinct words of nbits bits"""
    seen, out = set(), []
    while len(out) < count:
        w = tuple(int(b) for b in rng.integers(0, 2, nbits))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def random_cuts(rng, n, most):
    """cut points of a stream of n samples into pushes of 1 .. most samples"""
    cuts, at = [], 0
    while True:
        at += int(rng.integers(1, most + 1))
        if at >= n:
            return cuts
        cuts.append(at)


# ---- 1. the table past one wave ---------------------------------------------------------------------------------------------------------
WAVE_REPEATED = [3, 63, 64, 70, 127, 128, 159, 160, 3]
WAVE_ROWS, WAVE_REPEATS = [3, 63, 64, 70, 127, 128, 159], [3, 2, 2, 2, 2, 2, 2]


def table_past_one_wave(last_gap=RGAP, **more):
    """165 distinct 70-bit words (the pitch is 72), of which 160 find a row, then repeats of rows in the first, second and third
    batch of 64, on both sides of each batch seam, and of word 160, which found no row.
    cuts: "carry" inside word 100 behind its 66th bit, "table" behind word 165, "repeats" between the repeats of 70 and 127;
    "halves": eight cuts in the middle of words, every one with more than 64 rows in the table"""
    pos, kw = settings(max_frame_bits=70, max_distinct_frames=160, **more)
    base = distinct_words(np.random.default_rng(4181), 165, 70)
    sent = base + [base[i] for i in WAVE_REPEATED]
    x, at = words_stream(sent, last_gap)
    cuts = dict(carry=int(at[100]) + 66 * BIT, table=int(at[165]), repeats=int(at[169]),
                halves=[int(at[w]) + off for w, off in ((66, 3), (80, 250), (101, 499 - 4), (127, 1), (128, 77), (150, 300), (166, 8), (170, 123))])
    return Case(pos, kw, x, sent, cuts)


# ---- 2. mixed lengths, prefixes, single-bit differences --------------------------------------------------------------------------------
PREFIX_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 200]
FLIPPED = [0, 63, 64, 128]


def prefixes_and_flips():
    """one 200-bit string cut to PREFIX_LENGTHS, and its 129-bit prefix with one of the bits FLIPPED turned over; all once, then
    all in reverse order.  cuts: "passes" between the two passes"""
    pos, kw = settings(frame_bits=None, max_frame_bits=200, max_distinct_frames=64)
    full = tuple(int(b) for b in np.random.default_rng(4182).integers(0, 2, 200))
    once = [full[:n] for n in PREFIX_LENGTHS]
    for k in FLIPPED:
        w = list(full[:129])
        w[k] ^= 1
        once.append(tuple(w))
    sent = once + once[::-1]
    x, at = words_stream(sent)
    return Case(pos, kw, x, sent, dict(passes=int(at[len(once)])))


# ---- 3. the handle's limits, filled -------------------------------------------------------------------------------------------------------
def longest_frame():
    """a word of 16,384 bits, the same with one more bit (an overflow), and the word again.  cuts: "carry" behind bit 16,000 of
    the first word"""
    pos, kw = settings(max_frame_bits=16384, max_distinct_frames=256)
    w = tuple(int(b) for b in np.random.default_rng(4183).integers(0, 2, 16384))
    sent = [w, w + (1,), w]
    x, _ = words_stream(sent)
    return Case(pos, kw, x, sent, dict(carry=16000 * BIT))


FULL_REPEATED = [0, 1023, 1024, 63, 64]


def fullest_table():
    """1,030 distinct 12-bit words, of which 1,024 find a row, then repeats of the first and last row, of a word that found none
    and of both sides of the first batch seam.  cuts: "table" behind word 1,030"""
    pos, kw = settings(max_frame_bits=4096, max_distinct_frames=1024)
    base = [tuple(int(b) for b in np.binary_repr(int(v), 12)) for v in np.random.default_rng(4184).permutation(4096)[:1030]]
    sent = base + [base[i] for i in FULL_REPEATED]
    x, at = words_stream(sent)
    return Case(pos, kw, x, sent, dict(table=int(at[1030])))


# ---- 4. many deliveries in one push -----------------------------------------------------------------------------------------------------
def many_transmissions(count=200):
    """count transmissions of one to three words of 3 to 9 bits, some sent twice or three times, each ended by the reset gap.
    cuts: "random" pushes of 1 .. 3,000 samples"""
    pos, kw = settings()
    rng = np.random.default_rng(4185)
    parts, sent = [], []
    for _ in range(count):
        tx = []
        for w in distinct_words(rng, int(rng.integers(1, 4)), int(rng.integers(3, 10))):
            tx += [w] * int(rng.choice([1, 1, 2, 3]))
        tx = [tx[i] for i in rng.permutation(len(tx))]
        parts.append(words_stream(tx)[0])
        sent.append(tx)
    x = np.concatenate(parts)
    return Case(pos, kw, x, sent, dict(random=random_cuts(rng, len(x), 3000)))


# ---- 5. the fuzz family across tiles ---------------------------------------------------------------------------------------------------
def fuzz_tiled(seed, T=TILE):
    """pm.fuzz_case(seed) repeated until it is longer than 3 T + 17 samples: its jittered widths, NaN and Inf meet the tile seams
    at a different phase in every repetition.  cuts: "seams" one cut each, "random" pushes of 1 .. 700 samples"""
    pos, kw, x = pm.fuzz_case(seed)
    x = np.tile(x, -(-(3 * T + 17) // len(x)))
    rng = np.random.default_rng(5000 + seed)
    return Case(pos, kw, x, None, dict(seams=[T - 1, T, T + 1, 2 * T], random=random_cuts(rng, len(x), 700)))


def complex_of(x):
    """-> (z, power): Complex samples of amplitude sqrt(max(x, 0)) in f32 (NaN stays NaN, -Inf becomes 0), in the real part on
    even samples and in the imaginary part on odd ones, and numpy's f32 zr * zr + zi * zi, which ComplexToMag2 computes"""
    with np.errstate(invalid="ignore"):
        amp = np.sqrt(np.maximum(np.asarray(x, np.float32), np.float32(0))).astype(np.float32)
    even = np.arange(len(amp)) % 2 == 0
    zr, zi = np.where(even, amp, np.float32(0)).astype(np.float32), np.where(even, np.float32(0), amp).astype(np.float32)
    z = np.empty(len(amp), np.complex64)
    z.real, z.imag = zr, zi
    with np.errstate(invalid="ignore", over="ignore"):
        power = (zr * zr + zi * zi).astype(np.float32)
    return z, power
