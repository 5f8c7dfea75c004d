"""Test-side statements of BinarySlicer (src/binary_slicer.rs:17-19), NrziDecode / NrziEncode (src/nrzi.rs:36-69), the Lfsr of
Descrambler / Scrambler (src/descrambler.rs:13-48) and CorrelateAccessCodeTag (src/correlate_access_code.rs:93-118), written
as the reference's SEQUENTIAL state machines — the shift register with count_ones, `last`, the sliding list — so that they
share nothing with the GPU kernel's word-and-shift formulation.  Test infrastructure only: the product never imports it.

  slicer               x > 0.0
  Nrzi, Lfsr, Slide    the three state machines; every one keeps its state across run() calls
  Chain                slicer -> [^1] -> [Nrzi] -> [Lfsr descramble] -> [Slide] in the order of rr_bit_decoder_create
  descramble_unrolled  stage 4 of the kernel as a formula: s[n] = d[n] ^ XOR_j d[n-1-(len-j)] over the mask bits j <= len
  chain_vectorised     slicer -> NrziDecode -> Descrambler.g3ruh -> correlator on whole numpy arrays, for windows of millions of
                       samples; tests/test_bits_cpu.py holds it to Chain
  nrzi_encode, scramble, hdlc_stuff, ax25ish_symbols   building test signals
"""
from __future__ import annotations

import numpy as np

HDLC_FLAG = [0, 1, 1, 1, 1, 1, 1, 0]
G3RUH = (0x21, 0, 16)
IL2P_SYNC = [int(b) for b in f"{0xF15E48:024b}"]      # src/il2p_deframer.rs:16-18: the 24-bit sync word, oldest bit first
IL2P_SYNC32 = [0, 1, 0, 1, 0, 1, 0, 1] + IL2P_SYNC     # ... behind the last byte of its 0x55 preamble: a 32-bit code


def slicer(x):
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) > np.float32(0.0)).astype(np.uint8)


class Nrzi:
    """NrziDecode::process_sync (nrzi.rs:36-41)"""

    def __init__(self):
        self.last = 0

    def run(self, bits):
        out = []
        for a in bits:
            a = int(a)
            tmp, self.last = self.last, a
            out.append(1 ^ a ^ tmp)
        return out


class Lfsr:
    """descrambler.rs:13-48"""

    def __init__(self, mask, seed, length):
        assert length < 64
        self.mask, self.len, self.shift_reg = int(mask), int(length), int(seed)

    def next_descramble(self, i):
        assert i <= 1
        ret = 1 & (bin(self.shift_reg & self.mask).count("1") ^ i)
        self.shift_reg = (self.shift_reg >> 1) | (i << self.len)
        return ret

    def next_scramble(self, i):
        assert i <= 1
        ret = self.shift_reg & 1
        tmp = 1 & (bin(self.shift_reg & self.mask).count("1") ^ i)
        self.shift_reg = (self.shift_reg >> 1) | (tmp << self.len)
        return ret

    def run(self, bits):
        return [self.next_descramble(int(b)) for b in bits]


class Slide:
    """CorrelateAccessCodeTag::process_sync_tags (correlate_access_code.rs:93-118): (pos, diffs) of the tags, pos counted from
    the start of each run() call"""

    def __init__(self, code, allowed_diffs):
        assert len(code) > 0, "access code must be nonempty"
        self.code, self.allowed, self.slide = [int(c) for c in code], int(allowed_diffs), []

    def run(self, bits):
        tags = []
        for pos, a in enumerate(bits):
            self.slide.append(int(a))
            if len(self.slide) > len(self.code):
                self.slide.pop(0)
            diffs = sum(1 for x, y in zip(self.slide, self.code) if x != y)
            if len(self.slide) == len(self.code) and diffs <= self.allowed:
                tags.append((pos, diffs))
        return tags


class Chain:
    """the stages of rr_bit_decoder_create in its order; soft=False: u8 bits in (no slicer).  State carried across run()."""

    def __init__(self, invert=False, nrzi=False, descrambler=None, code=None, allowed_diffs=0, soft=True):
        self.soft, self.invert = soft, invert
        self.nrzi = Nrzi() if nrzi else None
        self.lfsr = Lfsr(*descrambler) if descrambler is not None else None
        self.slide = Slide(code, allowed_diffs) if code is not None and len(code) else None

    def run(self, x):
        """-> (bits uint8[], pos uint64[], diffs uint8[])"""
        b = slicer(x).tolist() if self.soft else [int(v) for v in x]
        if self.invert:
            b = [v ^ 1 for v in b]
        if self.nrzi:
            b = self.nrzi.run(b)
        if self.lfsr:
            b = self.lfsr.run(b)
        tags = self.slide.run(b) if self.slide else []
        return (np.array(b, np.uint8), np.array([t[0] for t in tags], np.uint64), np.array([t[1] for t in tags], np.uint8))


def descramble_unrolled(d, mask, seed, length):
    """stage 4 as the kernel states it: no register, only earlier inputs; d[-1-k] = bit (length-k) of seed, k = 0..length"""
    d = [int(v) for v in d]

    def at(i):
        return d[i] if i >= 0 else (seed >> (length - (-1 - i))) & 1

    out = []
    for n in range(len(d)):
        s = d[n]
        for j in range(length + 1):
            if mask >> j & 1:
                s ^= at(n - 1 - (length - j))
        out.append(s)
    return out


def chain_vectorised(x, code, allowed_diffs=0):
    """-> (bits, pos, diffs) of Chain(nrzi=True, descrambler=G3RUH, code=code, allowed_diffs=...) on a stream that starts at
    x[0], as shifts of whole arrays (seed 0, last 0: everything before the stream is 0)"""
    def back(a, k):
        out = np.zeros_like(a)
        out[k:] = a[:len(a) - k]
        return out

    r = slicer(x)
    d = np.uint8(1) ^ r ^ back(r, 1)
    s = d ^ back(d, 12) ^ back(d, 17)
    L = len(code)
    diffs = np.zeros(len(s), np.uint8)
    for k, c in enumerate(code):
        diffs += back(s, L - 1 - k) != np.uint8(c)
    ok = diffs <= allowed_diffs
    ok[:L - 1] = False
    pos = np.nonzero(ok)[0].astype(np.uint64)
    return s, pos, diffs[ok]


def nrzi_encode(bits, state=0):
    """NrziEncode::process_sync (nrzi.rs:63-69)"""
    out = []
    for a in bits:
        if int(a) == 0:
            state ^= 1
        out.append(state)
    return out


def scramble(bits, mask=0x21, seed=0, length=16):
    l = Lfsr(mask, seed, length)
    return [l.next_scramble(int(b)) for b in bits]


def hdlc_stuff(bits):
    out, ones = [], 0
    for b in bits:
        out.append(int(b))
        ones = ones + 1 if b else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return out


def ax25ish_symbols(n_frames, seed):
    """-> (soft symbols f32[], planted uint64[]): n_frames transmissions, each two opening flags, stuffed random payload, one
    closing flag; NRZI-encoded, G3RUH-scrambled by a transmitter that keys up afresh (its register's 17 zeros go out first),
    mapped to +-1 plus noise of sigma 0.2, with stretches of pure noise in between.  planted: the positions in the DECODED
    stream (slicer -> NrziDecode -> Descrambler.g3ruh) of the last bit of every flag but each frame's first, whose leading
    bit needs a sample from before the transmission."""
    rng = np.random.default_rng(seed)
    parts, planted, at = [], [], 0

    def noise(n):
        nonlocal at
        parts.append(rng.normal(0.0, 0.2, n).astype(np.float32))
        at += n

    noise(int(rng.integers(50, 300)))
    for _ in range(n_frames):
        payload = hdlc_stuff(rng.integers(0, 2, int(rng.integers(100, 400))).tolist())
        tx = HDLC_FLAG + HDLC_FLAG + payload + HDLC_FLAG
        ends = [15, len(tx) - 1]
        line = scramble(nrzi_encode(tx) + [0] * 17)           # the scrambler delays by len + 1 = 17
        sym = (2.0 * np.array(line, np.float64) - 1.0) + np.clip(rng.normal(0.0, 0.2, len(line)), -0.8, 0.8)
        parts.append(sym.astype(np.float32))
        planted += [at + 17 + e for e in ends]
        at += len(line)
        noise(int(rng.integers(100, 600)))
    return np.concatenate(parts), np.array(planted, np.uint64)
