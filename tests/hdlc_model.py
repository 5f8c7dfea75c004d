"""HdlcDeframer (src/hdlc_deframer.rs) twice over: the specification a device deframer is to be held against.

HdlcModel is the reference's machine as it is written: one bit at a time through Unsynced(register) / Synced(ones, bits) /
FinalCheck(bits), find_right_crc with its flip order, the three counters.  It keeps its state between run() calls.

deframe_events() is a data-parallel formulation of the same behaviour: flag ends, aborts and stuffed bits as local features of the
raw bits, one 3 -> 3 map over {S, U, U3} per gap between two flag ends, the chain of maps resolved, one candidate frame per
emitting gap, and the single-bit repair as a search by CRC syndrome.  It shares no code with HdlcModel;
tests/test_hdlc_cpu.py holds the two against each other.
"""
import numpy as np

POLY = 0x8408          # CRC-16/X.25: reflected 0x1021, init 0xffff, final xor 0xffff


def _crc_table():
    t = []
    for b in range(256):
        v = b
        for _ in range(8):
            v = (v >> 1) ^ (POLY if v & 1 else 0)
        t.append(v)
    return t


_TABLE = _crc_table()


def crc16_x25(data) -> int:
    fcs = 0xffff
    for b in bytes(data):
        fcs = (fcs >> 8) ^ _TABLE[(fcs ^ b) & 0xff]
    return fcs ^ 0xffff


def find_right_crc(data: bytes, got: int, fix_bits: bool):
    """-> (new data or None, crc, fixed) as hdlc_deframer.rs:41-71"""
    crc = crc16_x25(data)
    if got == crc or not fix_bits:
        return None, crc, False
    copy = bytearray(data)
    for byte in range(len(copy)):
        for bit in range(8):
            copy[byte] ^= 1 << bit
            c = crc16_x25(copy)
            if c == got:
                return bytes(copy), c, True
            copy[byte] ^= 1 << bit
    for crcbit in range(16):
        if got ^ (1 << crcbit) == crc:
            return None, got ^ (1 << crcbit), True
    return None, crc, False


_TABLE_NP = np.array(_TABLE, np.uint32)


def find_right_crc_lockstep(data: bytes, got: int, fix_bits: bool):
    """find_right_crc for long bodies: the same table CRC of the same 8 N single-flip copies, all of them stepped together byte
    by byte (copy h is the data with bit h & 7 of byte h >> 3 flipped), and the first copy in find_right_crc's order that
    matches.  Each copy's CRC is computed in full; nothing is derived from another copy's."""
    crc = crc16_x25(data)
    if got == crc or not fix_bits:
        return None, crc, False
    n = len(data)
    if n:
        fcs = np.full(8 * n, 0xffff, np.uint32)
        masks = 1 << np.arange(8, dtype=np.uint32)
        for i, b in enumerate(bytes(data)):
            idx = (fcs ^ b) & 0xff
            idx[8 * i:8 * i + 8] ^= masks
            fcs = (fcs >> 8) ^ _TABLE_NP[idx]
        hits = np.flatnonzero((fcs ^ 0xffff) == got)
        if len(hits):
            h = int(hits[0])
            copy = bytearray(data)
            copy[h >> 3] ^= 1 << (h & 7)
            return bytes(copy), got, True
    for crcbit in range(16):
        if got ^ (1 << crcbit) == crc:
            return None, got ^ (1 << crcbit), True
    return None, crc, False


class HdlcModel:
    """the sequential machine; frames are (packet_pos, bytes, bitfixed).  `repair` stands in for find_right_crc (same arguments,
    same result: find_right_crc_lockstep where bodies are long)"""
    UNSYNCED, SYNCED, FINAL = 0, 1, 2

    def __init__(self, min_size, max_size, keep_checksum=False, fix_bits=False, repair=find_right_crc):
        self.min_size, self.max_size, self.keep, self.fix = min_size, max_size, keep_checksum, fix_bits
        self.repair = repair
        self.state, self.reg, self.ones, self.bits = self.UNSYNCED, 0xff, 0, []
        self.decoded = self.crc_error = self.bitfixed = 0
        self.pos = 0

    def _unsync(self):
        self.state, self.reg, self.bits = self.UNSYNCED, 0xff, []

    def _sync(self):
        self.state, self.ones, self.bits = self.SYNCED, 0, []

    def _step(self, bit, pos, out):
        if self.state == self.UNSYNCED:
            n = (self.reg >> 1) | (bit << 7)
            if n == 0x7e:
                self._sync()
            else:
                self.reg = n
        elif self.state == self.SYNCED:
            if len(self.bits) > self.max_size * 8:
                return self._unsync()
            if bit:
                self.bits.append(1)
                if self.ones == 5:
                    self.state = self.FINAL
                else:
                    self.ones += 1
            elif self.ones == 5:
                self.ones = 0
            else:
                self.bits.append(0)
                self.ones = 0
        else:
            if bit == 1 or len(self.bits) < 7:
                return self._unsync()
            bits = self.bits[:-7]
            self._sync()
            if len(bits) % 8 or len(bits) // 8 < self.min_size:
                return
            data = bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))
            if self.keep:
                self.decoded += 1
                out.append((pos, data, False))
                return
            if len(data) < 2:
                return
            body, got = data[:-2], data[-2] | data[-1] << 8
            new, crc, fixed = self.repair(body, got, self.fix)
            if fixed:
                self.bitfixed += 1
            if new is not None:
                body = new
            if crc != got:
                self.crc_error += 1
                return
            self.decoded += 1
            out.append((pos, body, fixed))

    def run(self, bits):
        """the frames that ended inside `bits` (a sequence of bytes: the lowest bit of each is the bit)"""
        out = []
        for b in np.asarray(bits, np.uint8).tolist():
            self._step(b & 1, self.pos, out)
            self.pos += 1
        return out

    def stats(self):
        return self.decoded, self.crc_error, self.bitfixed


S, U, U3 = 0, 1, 2


def deframe_events(bits, min_size, max_size, keep_checksum=False, fix_bits=False):
    """-> (frames, (decoded, crc_error, bitfixed)) of the whole stream `bits`, by the flag-to-flag formulation"""
    b = (np.asarray(bits, np.uint8) & 1).astype(np.int64)
    n = len(b)
    pad = np.concatenate([np.zeros(8, np.int64), b])           # pad[p + 8 - k] = b[p - k]
    back = lambda k: pad[8 - k:8 - k + n]
    pos = np.arange(n)
    flag = (b == 0) & (back(7) == 0) & (pos >= 7)
    for k in range(1, 7):
        flag &= back(k) == 1
    ones5 = np.ones(n, bool)
    for k in range(1, 6):
        ones5 &= (back(k) == 1) & (pos >= k)
    run6 = ones5 & (back(6) == 1) & (pos >= 6)
    abort = (b == 1) & run6                                     # the seventh 1 in a row
    stuffed = (b == 0) & ones5 & ~run6                          # run == 5 exactly
    cum_st = np.concatenate([[0], np.cumsum(stuffed)])          # cum_st[p] = stuffed bits in [0, p)
    ab_pos = np.flatnonzero(abort)
    ends = np.flatnonzero(flag)
    frames, decoded, crc_error, bitfixed = [], 0, 0, 0
    state = U
    for j, f in enumerate(ends.tolist()):
        if j == 0:
            state = S
            continue
        s = ends[j - 1]
        share = f == s + 7
        if state == U:
            state = S
            continue
        if state == U3:
            state = U if share else S
            continue
        k = np.searchsorted(ab_pos, s + 1)
        a = int(ab_pos[k]) if k < len(ab_pos) and ab_pos[k] < f else None
        # collected before bit q: (q - 1 - s) - stuffed(s+1 .. q-1), nondecreasing in q
        qs = np.arange(s + 1, f)
        coll = (qs - 1 - s) - (cum_st[qs] - cum_st[s + 1])
        over = np.flatnonzero(coll > 8 * max_size)
        q = int(qs[over[0]]) if len(over) else None
        r = min(x for x in (a, q) if x is not None) if (a is not None or q is not None) else None
        if r is not None:
            state = S if r < f - 7 else U
            continue
        if share:
            state = U3
            continue
        state = S
        kept = b[s + 1:f][~stuffed[s + 1:f]]
        L = len(kept) - 7
        if L % 8 or L // 8 < min_size:
            continue
        kept = kept[:L].tolist()
        data = bytes(sum(kept[i + k] << k for k in range(8)) for i in range(0, L, 8))
        if keep_checksum:
            decoded += 1
            frames.append((f, data, False))
            continue
        if len(data) < 2:
            continue
        body, got = data[:-2], data[-2] | data[-1] << 8
        diff = crc16_x25(body) ^ got
        if diff == 0:
            decoded += 1
            frames.append((f, body, False))
        elif not fix_bits:
            crc_error += 1
        else:
            # the CRC is linear: flipping the data bit d bits before the end changes it by syn(d), whatever the data
            N, hit, v = 8 * len(body), None, 1
            for d in range(1, N + 1):
                v = (v >> 1) ^ (POLY if v & 1 else 0)
                if v == diff:
                    hit = N - d                                 # (at most one: N is below the polynomial's period)
            if hit is not None:
                fixed = bytearray(body)
                fixed[hit // 8] ^= 1 << (hit % 8)
                bitfixed += 1
                decoded += 1
                frames.append((f, bytes(fixed), True))
            elif bin(diff).count("1") == 1:
                bitfixed += 1
                crc_error += 1
            else:
                crc_error += 1
    return frames, (decoded, crc_error, bitfixed)


# ---- building streams ------------------------------------------------------------------------------------------------
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def bytes_to_bits(data):
    return [(x >> k) & 1 for x in bytes(data) for k in range(8)]


def stuff(bits):
    out, run = [], 0
    for x in bits:
        out.append(x)
        run = run + 1 if x else 0
        if run == 5:
            out.append(0)
            run = 0
    return out


def frame_bits(payload: bytes, flags_before=1, flags_after=1, with_crc=True):
    """flags, the stuffed payload (+ its checksum), flags"""
    body = bytes(payload)
    if with_crc:
        c = crc16_x25(body)
        body += bytes([c & 0xff, c >> 8])
    return FLAG * flags_before + stuff(bytes_to_bits(body)) + FLAG * flags_after


def draw_stream(rng, nbits, p_frame=0.5):
    """random, ones-heavy and flag-heavy pieces and whole frames, about nbits long"""
    out = []
    while len(out) < nbits:
        kind = rng.integers(0, 7)
        m = int(rng.integers(1, 40))
        if kind == 0:
            out += rng.integers(0, 2, m).tolist()
        elif kind == 1:
            out += (rng.random(m) < 0.85).astype(int).tolist()
        elif kind == 2:
            out += FLAG * int(rng.integers(1, 4))
        elif kind == 3:
            out += FLAG[:7] * int(rng.integers(1, 5)) + [0]          # flags sharing their zeros
        elif kind == 4:
            out += [1] * int(rng.integers(5, 9)) + [0]
        else:
            payload = rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes()
            fb = frame_bits(payload, 1, int(rng.integers(0, 2)), with_crc=bool(rng.integers(0, 2)))
            if rng.random() < 0.3 and len(fb) > 16:
                fb[int(rng.integers(8, len(fb) - 8))] ^= 1
            out += fb
    return np.array(out[:nbits], np.uint8)
