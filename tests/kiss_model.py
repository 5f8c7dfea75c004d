"""What the tests of rr.KissDecode / rr.KissEncode share (include/rustradio_amd.h).  Test infrastructure only; nothing
here touches the GPU.

Two statements of KissFrame -> KissDecode (src/kiss.rs:96-228):
  SequentialDecoder    the two blocks byte by byte, as their work() loops run (the back-pressure apart)
  ClosedDecoder        the closed form over FEND positions the device block is built on
and one of KissEncode -> PduToStream (:247-286): encode().

A packet is (pos, port, in_bytes, bytes): pos = the stream position of the closing FEND.  The counters are
(frames, delivered, nondata, bad_escape, overlong); an over-long gap counts at the FEND that closes it."""
import json
import os

import numpy as np

FEND, FESC, TFEND, TFESC = 0xC0, 0xDB, 0xDC, 0xDD      # src/kiss.rs:7-10
MAX_LEN = 10000                                         # :6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kiss_known_answers.json")


def known_answers():
    with open(GOLDEN) as f:
        return json.load(f)


def unescape(x: bytes):
    """unescape (:47-77) -> (bytes, None) or (None, which error): "invalid" (a FESC followed by a wrong byte; a FEND cannot
    occur inside a frame) or "trailing" (ended on an escape)"""
    out, esc = bytearray(), False
    for b in x:
        if esc:
            if b == TFESC:
                out.append(FESC)
            elif b == TFEND:
                out.append(FEND)
            else:
                return None, "invalid"
            esc = False
        elif b == FESC:
            esc = True
        else:
            out.append(b)
    if esc:
        return None, "trailing"
    return bytes(out), None


def encode_one(packet: bytes, port: int = 0) -> bytes:
    """KissEncode's port rule (:256-266) and escape (:30-44)"""
    port = port if 0 <= port < 16 else 0
    out = bytearray([FEND, (port << 4) & 0xFF])
    for b in packet:
        if b == FEND:
            out += bytes([FESC, TFEND])
        elif b == FESC:
            out += bytes([FESC, TFESC])
        else:
            out.append(b)
    out.append(FEND)
    return bytes(out)


def encode(packets, ports=None) -> bytes:
    """the frames back to back (PduToStream)"""
    ports = [0] * len(packets) if ports is None else ports
    return b"".join(encode_one(p, q) for p, q in zip(packets, ports))


def encode_records(packets, ports=None):
    """[(start, len, escaped, port)] of encode()"""
    ports = [0] * len(packets) if ports is None else ports
    out, at = [], 0
    for p, q in zip(packets, ports):
        esc = sum(1 for b in bytes(p) if b in (FEND, FESC))
        out.append((at, 3 + len(p) + esc, esc, q if 0 <= q < 16 else 0))
        at += 3 + len(p) + esc
    return out


class _Counters:
    def __init__(self):
        self.frames = self.delivered = self.nondata = self.bad_escape = self.overlong = 0
        self.bad_trailing = self.bad_invalid = 0            # the two kinds of bad escape (not an ABI counter)

    def stats(self):
        return (self.frames, self.delivered, self.nondata, self.bad_escape, self.overlong)

    def _decode(self, frame: bytes, pos: int, out: list):
        """KissDecode::work for one KissFrame output (:105-135; strip_fend has nothing to strip: a frame holds no FEND)"""
        self.frames += 1
        port, x = frame[0], frame[1:]
        if port & 0xF:
            self.nondata += 1
            return
        o, err = unescape(x)
        if o is None:
            self.bad_escape += 1
            if err == "trailing":
                self.bad_trailing += 1
            else:
                self.bad_invalid += 1
            return
        self.delivered += 1
        out.append((pos, (port >> 4) & 0xF, len(x), o))


class SequentialDecoder(_Counters):
    """KissFrame's state machine byte by byte (:165-228) with KissDecode behind it"""

    def __init__(self, max_len: int = MAX_LEN):
        super().__init__()
        self.max_len = max_len
        self.synced = False
        self.v = bytearray()
        self.dropped = False          # Unsynced because v outgrew max_len: the next FEND closes an over-long gap
        self.pos = 0

    def push(self, data: bytes):
        out = []
        for b in bytes(data):
            if not self.synced:
                if b == FEND:
                    if self.dropped:
                        self.overlong += 1
                        self.dropped = False
                    self.synced = True
                    self.v = bytearray()
            elif b == FEND:
                if self.v:
                    self._decode(bytes(self.v), self.pos, out)
                    self.v = bytearray()
            else:
                self.v.append(b)
                if len(self.v) > self.max_len:
                    self.synced, self.dropped, self.v = False, True, bytearray()
            self.pos += 1
        return out


class ClosedDecoder(_Counters):
    """The closed form: with f_0 < f_1 < ... the FEND positions of the whole stream, every gap b[f_j + 1 .. f_j+1) of 1 .. max_len
    bytes is a frame; a frame is bad exactly when some FESC of x = G[1:] is its last byte or is followed by a byte other than
    TFEND / TFESC; else the packet is x without its FESC bytes, the byte behind each mapped."""

    def __init__(self, max_len: int = MAX_LEN):
        super().__init__()
        self.max_len = max_len
        self.stream = bytearray()
        self.last_fend = None          # position of the latest FEND
        self.pos = 0

    def push(self, data: bytes):
        out = []
        data = bytes(data)
        self.stream += data
        a = np.frombuffer(data, np.uint8)
        for rel in np.flatnonzero(a == FEND):
            e = self.pos + int(rel)
            if self.last_fend is not None:
                g = bytes(self.stream[self.last_fend + 1:e])
                if len(g) > self.max_len:
                    self.overlong += 1
                elif len(g) >= 1:
                    self._closed(g, e, out)
            self.last_fend = e
        self.pos += len(data)
        return out

    def _closed(self, g: bytes, e: int, out: list):
        self.frames += 1
        if g[0] & 0xF:
            self.nondata += 1
            return
        x = np.frombuffer(g[1:], np.uint8)
        esc = x == FESC
        nxt = np.append(x[1:], FEND)                        # what stands behind each byte: the closing FEND behind the last
        bad = esc & (nxt != TFEND) & (nxt != TFESC)
        if bad.any():
            self.bad_escape += 1
            if bad[-1]:
                # unescape reports the first error it meets; the last byte is the first error only when no earlier one is bad
                if not bad[:-1].any():
                    self.bad_trailing += 1
                else:
                    self.bad_invalid += 1
            else:
                self.bad_invalid += 1
            return
        behind = np.append(False, esc[:-1])                 # the byte stands behind a FESC
        y = x.copy()
        y[behind & (x == TFEND)] = FEND
        y[behind & (x == TFESC)] = FESC
        self.delivered += 1
        out.append((e, g[0] >> 4, len(x), y[~esc].tobytes()))


def run(decoder, pushes):
    """-> (the packets of every push, the counters behind the last)"""
    return [decoder.push(p) for p in pushes], decoder.stats()


def draw_stream(rng, n: int, special: float = 0.55) -> bytes:
    """n bytes, `special` of them from the four special bytes and data ports; half of the others have a low nibble of 0, so that
    a frame's first byte is a data port often enough"""
    pick = rng.random(n)
    out = rng.integers(0, 256, n, dtype=np.uint8)
    out[rng.random(n) < 0.5] &= 0xF0
    sp = np.array([FEND, FEND, FEND, FESC, FESC, TFEND, TFESC, 0x00, 0x00, 0x10, 0x30], np.uint8)
    m = pick < special
    out[m] = sp[rng.integers(0, len(sp), int(m.sum()))]
    return out.tobytes()


def split(rng, data: bytes, k: int):
    """data in k pushes at drawn cuts (pushes of nothing included)"""
    cuts = sorted(int(c) for c in rng.integers(0, len(data) + 1, k - 1))
    edges = [0] + cuts + [len(data)]
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def encode_numpy(arena: np.ndarray, starts, lens, ports=None) -> np.ndarray:
    """encode() of the packets arena[starts[p] : starts[p] + lens[p]] with no loop over packets or bytes: what one host core does
    to a downloaded arena (tools/kiss_probe.py times it)"""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    P = len(lens)
    pb = np.concatenate(([0], np.cumsum(lens)))
    pk = np.repeat(np.arange(P), lens)                     # the packet of every payload byte
    g = np.arange(pb[-1])
    b = np.asarray(arena, np.uint8)[starts[pk] + (g - pb[pk])]
    esc = (b == FEND) | (b == FESC)
    C = np.concatenate(([0], np.cumsum(esc)))              # the escaped bytes in front of every payload byte
    out = np.empty(3 * P + pb[-1] + C[-1], np.uint8)
    at = 3 * pk + 2 + g + C[:-1]
    out[at] = np.where(esc, FESC, b)
    out[at[esc] + 1] = np.where(b[esc] == FEND, TFEND, TFESC)
    head = 3 * np.arange(P) + pb[:-1] + C[pb[:-1]]
    po = np.zeros(P, np.int64) if ports is None else np.asarray(ports, np.int64)
    out[head] = FEND
    out[head + 1] = np.where(po < 16, po << 4, 0) & 0xFF
    out[head + 2 + lens + (C[pb[1:]] - C[pb[:-1]])] = FEND
    return out


def decode_numpy(stream: np.ndarray, max_len: int = MAX_LEN):
    """the closed form over a whole stream with no loop over frames or bytes -> (pos, port, in_bytes, len, the packets' bytes
    packed in stream order)"""
    s = np.asarray(stream, np.uint8)
    f = np.flatnonzero(s == FEND)
    if len(f) < 2:
        return (np.zeros(0, np.int64),) * 4 + (np.zeros(0, np.uint8),)
    esc = s == FESC
    nxt = np.append(s[1:], 0)
    bad = esc & (nxt != TFEND) & (nxt != TFESC)
    E, B = np.concatenate(([0], np.cumsum(esc))), np.concatenate(([0], np.cumsum(bad)))
    a, e = f[:-1], f[1:]
    glen = e - a - 1
    ok = (glen >= 1) & (glen <= max_len)
    a, e, glen = a[ok], e[ok], glen[ok]
    port = s[a + 1]
    ok = ((port & 0xF) == 0) & (B[e] == B[a + 2])
    a, e, glen, port = a[ok], e[ok], glen[ok], port[ok]
    keep = np.zeros(len(s) + 1, np.int32)                  # +1 at the first byte of every delivered x, -1 at its closing FEND
    np.add.at(keep, a + 2, 1)
    np.add.at(keep, e, -1)
    inside = np.cumsum(keep[:-1]) > 0
    behind = np.append(False, esc[:-1]) & inside
    y = s.copy()
    y[behind & (s == TFEND)] = FEND
    y[behind & (s == TFESC)] = FESC
    return e, port >> 4, glen - 1, glen - 1 - (E[e] - E[a + 2]), y[inside & ~esc]
