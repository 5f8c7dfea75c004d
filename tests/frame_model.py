"""The transmit chain FcsAdder -> HdlcFramer -> PduToStream<u8> -> [Scrambler::g3ruh] -> [NrziEncode] -> [Map] twice over: the
specification rr_hdlc_framer, rr_scrambler_g3ruh and rr_nrzi_encode are held against.  Test infrastructure only.

FramerSeq is the reference's chain as it is written: calc_crc's table loop (hdlc_model.crc16_x25), hdlc_encode's loop with its
`ones` counter (src/hdlc_framer.rs:60-86), the Lfsr's register (bits_model.Lfsr.next_scramble) and NrziEncode's `out`
(bits_model.nrzi_encode).  It keeps the register and the level between push() calls.

closed_form() states the same behaviour without any of those loops: the CRC as a bit-serial division by x^16 + x^12 + x^5 + 1 in
the order of transmission, stuffing from the runs of ones (a run of r ones gets floor(r / 5) stuffed bits, behind every fifth),
the scrambler as a product of shifted XORs, NRZI as a cumulative parity.  It shares no code with FramerSeq;
tests/test_frame_cpu.py holds the two against each other.
"""
import numpy as np

import bits_model as bm
import hdlc_model as hm

FCS, G3RUH, NRZI, SYMBOLS = 1, 2, 4, 8
SYNC = [0, 1, 1, 1, 1, 1, 1, 0]
SYNC_BYTES = 20


def bound(flags, lens):
    """rr_hdlc_framer_bound"""
    return sum(320 + 8 * (n + (2 if flags & FCS else 0)) + 8 * (n + (2 if flags & FCS else 0)) // 5 for n in lens)


# ---- the reference's loops ----------------------------------------------------------------------------------------------------------------
def fcs_adder(data: bytes) -> bytes:
    crc = hm.crc16_x25(data)
    return bytes(data) + bytes([crc & 0xff, (crc >> 8) & 0xff])


def hdlc_encode(data: bytes):
    """-> (bits, stuffed)"""
    out = []
    for _ in range(SYNC_BYTES):
        out.extend(SYNC)
    ones = stuffed = 0
    for byte in bytes(data):
        for _ in range(8):
            if byte & 1 == 1:
                ones += 1
                out.append(1)
                if ones == 5:
                    ones = 0
                    out.append(0)
                    stuffed += 1
            else:
                ones = 0
                out.append(0)
            byte >>= 1
    for _ in range(SYNC_BYTES):
        out.extend(SYNC)
    return out, stuffed


class FramerSeq:
    def __init__(self, flags=0, lo=-1.0, hi=1.0):
        self.flags, self.lo, self.hi = flags, np.float32(lo), np.float32(hi)
        self.lfsr = bm.Lfsr(*bm.G3RUH)
        self.level = 0

    def line(self, bits):
        """Scrambler::g3ruh -> NrziEncode over the next bits of the stream"""
        if self.flags & G3RUH:
            bits = [self.lfsr.next_scramble(int(b) & 1) for b in bits]
        if self.flags & NRZI:
            bits = bm.nrzi_encode(bits, self.level)
            if bits:
                self.level = bits[-1]
        return bits

    def push(self, packets):
        """-> (out: uint8[] or float32[], records: [(start, len, stuffed, fcs)])"""
        stream, recs = [], []
        for p in packets:
            p = bytes(p)
            fcs = hm.crc16_x25(p) if self.flags & FCS else 0
            bits, stuffed = hdlc_encode(fcs_adder(p) if self.flags & FCS else p)
            recs.append((len(stream), len(bits), stuffed, fcs))
            stream += bits                       # PduToStream: the packets back to back, `start` tagged at each first bit
        out = np.array(self.line(stream), np.uint8)
        if self.flags & SYMBOLS:
            out = np.where(out != 0, self.hi, self.lo).astype(np.float32)
        return out, recs


# ---- the closed form ----------------------------------------------------------------------------------------------------------------------
def bits_lsb_first(data: bytes) -> np.ndarray:
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little") if len(data) else np.zeros(0, np.uint8)


def crc_by_division(data: bytes) -> int:
    """CRC-16/X.25 on the bits in the order they are sent: register 0xffff, generator x^16 + x^12 + x^5 + 1, complemented, and
    read back with the first-sent bit lowest"""
    reg = 0xffff
    for b in bits_lsb_first(data).tolist():
        top = ((reg >> 15) & 1) ^ b
        reg = (reg << 1) & 0xffff
        if top:
            reg ^= 0x1021
    reg ^= 0xffff
    return int(f"{reg:016b}"[::-1], 2)


def stuff_closed(bits: np.ndarray):
    """-> (stuffed bit array, number of stuffed bits): a 0 goes behind every one whose place in its run of ones is a multiple of 5"""
    n = len(bits)
    if n == 0:
        return bits.copy(), 0
    idx = np.arange(n)
    last_zero = np.maximum.accumulate(np.where(bits == 0, idx, -1))
    place = idx - last_zero                                   # 1, 2, 3 .. inside a run of ones, 0 at a zero
    after = (bits == 1) & (place % 5 == 0)
    before = np.cumsum(after) - after                         # stuffed bits in front of each payload bit
    out = np.zeros(n + int(after.sum()), np.uint8)
    out[idx + before] = bits
    return out, int(after.sum())


def back(a, k):
    out = np.zeros_like(a)
    if k < len(a):
        out[k:] = a[:len(a) - k]
    return out


def scramble_closed(bits: np.ndarray) -> np.ndarray:
    """1 / (1 + x^12 + x^17) over GF(2) as the product of (1 + x^(12 2^k) + x^(17 2^k)), then the register's 17 bits of delay"""
    a = bits.astype(np.uint8).copy()
    k = 0
    while 12 << k < len(a):
        a = a ^ back(a, 12 << k) ^ back(a, 17 << k)
        k += 1
    return back(a, 17)


def nrzi_closed(bits: np.ndarray) -> np.ndarray:
    return (np.cumsum(1 - bits.astype(np.int64)) & 1).astype(np.uint8)


def closed_form(packets, flags, lo=-1.0, hi=1.0):
    """the whole stream of `packets` from the start of the stream -> (out, records)"""
    flag = np.tile(np.array(SYNC, np.uint8), SYNC_BYTES)
    parts, recs, at = [], [], 0
    for p in packets:
        p = bytes(p)
        fcs = crc_by_division(p) if flags & FCS else 0
        body = p + bytes([fcs & 0xff, fcs >> 8]) if flags & FCS else p
        st, stuffed = stuff_closed(bits_lsb_first(body))
        n = 2 * len(flag) + len(st)
        recs.append((at, n, stuffed, fcs))
        parts += [flag, st, flag]
        at += n
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if flags & G3RUH:
        out = scramble_closed(out)
    if flags & NRZI:
        out = nrzi_closed(out)
    if flags & SYMBOLS:
        out = np.where(out != 0, np.float32(hi), np.float32(lo)).astype(np.float32)
    return out, recs


def draw_packets(rng, npackets, max_len, p_one=0.9):
    """packets of 0 .. max_len bytes whose bits are 1 with probability p_one: stuffing is frequent"""
    out = []
    for _ in range(npackets):
        n = int(rng.integers(0, max_len + 1))
        out.append(np.packbits((rng.random(8 * n) < p_one).astype(np.uint8), bitorder="little").tobytes() if n else b"")
    return out
