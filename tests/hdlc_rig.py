"""What the GPU tests of rr_hdlc_deframer share: handles paired with the sequential machine of tests/hdlc_model.py, and the
host-side view of a stream (its flag ends, what a handle carries) that the tests use to show which loop an input reaches."""
import numpy as np
import torch

import hdlc_model as hm
import rustradio_amd as rr

KEEP, FIX = rr.HDLC_KEEP_CHECKSUM, rr.HDLC_FIX_BITS
HALO = 8                # bits a handle carries in front of the open gap (hdlc_core.hpp HDLC_HALO)


def to_dev(x):
    """a host array of bits -> (device tensor, its raw pointer); a tensor of one byte for no bits, so that the pointer is real"""
    t = torch.from_numpy(x.copy()).cuda() if len(x) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr()


class Rig:
    """one handle per configuration, each paired with an HdlcModel that is fed the same bits"""

    def __init__(self, configs, repair=hm.find_right_crc):
        self.dev = {c: rr.HdlcDeframer(*c) for c in configs}
        self.model = {c: hm.HdlcModel(c[0], c[1], bool(c[2] & KEEP), bool(c[2] & FIX), repair) for c in configs}

    def feed(self, cfg, bits, via="push"):
        """the same bits into the handle and its model -> the frames, which must agree, as must the counters"""
        x = np.ascontiguousarray(bits, np.uint8)
        want = self.model[cfg].run(x)
        d = self.dev[cfg]
        if via == "push":
            got = d.push(x)
        else:
            t, p = to_dev(x)
            d.push_dev(p, len(x))
            got = d.result()
        assert got == want, (cfg, len(x), got[:3], want[:3])
        assert d.stats() == self.model[cfg].stats(), cfg
        return got

    def reset(self, cfg):
        """16 ones: the model Unsynced(0xff), nothing emitted.  The handle agrees from here on, but it has not looked at the open
        gap yet: if the stream so far left it in S it carries that gap and these ones behind it, not 8 bits (see clear())."""
        assert self.feed(cfg, [1] * 16) == []
        m = self.model[cfg]
        assert (m.state, m.reg, m.bits) == (m.UNSYNCED, 0xff, [])

    def clear(self, cfg):
        """reset(), and the handle carries its 8 halo bits and nothing else, so that bit i of the next push is virtual bit 8 + i.
        The ones abort whatever was open, which makes the first of three flags sharing their zeros an S, the second a U3 and
        the third a U whatever the handle was in; behind a U only the last 8 bits are carried (hdlc_carry_plan)."""
        assert self.feed(cfg, [1] * 16 + hm.FLAG[:7] * 3 + [0] + [1] * 8) == []
        m = self.model[cfg]
        assert (m.state, m.reg, m.bits) == (m.UNSYNCED, 0xff, [])


def flag_ends(bits):
    """the positions at which 0 111111 0 ends"""
    b = np.asarray(bits, np.uint8) & 1
    n = len(b)
    if n < 8:
        return np.zeros(0, np.int64)
    m = (b[7:] == 0) & (b[:n - 7] == 0)
    for k in range(1, 7):
        m &= b[7 - k:n - k] == 1
    return np.flatnonzero(m) + 7


def reach(max_size):
    """hdlc_core.hpp hdlc_reach: a gap of more raw bits has left Synced whatever it holds"""
    m = 8 * max_size + 1
    return m + (m - 1) // 5 + 8


def carried_at_least(stream, model):
    """A lower bound of the bits a handle carries behind `stream`, all the bits it has seen since clear(), from the state of the
    model that saw them too.  While the model collects, the handle is in S at the last flag end and keeps the 8 bits up to it
    and the whole open gap, unless that is longer than hdlc_reach; otherwise it keeps at least the 8 bits of the halo."""
    ends = flag_ends(stream)
    if model.state == model.UNSYNCED or not len(ends):
        return HALO
    gap = len(stream) - 1 - int(ends[-1])
    return HALO + gap if gap <= reach(model.max_size) else HALO


def bits_of(data):
    """bytes -> bits, the lowest first (hdlc_model.bytes_to_bits as an array)"""
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little")


def stuffed_ones(n):
    """n raw bits of a stuffed run of ones: no flag, no abort"""
    return np.resize(np.array([1, 1, 1, 1, 1, 0], np.uint8), n)


FLAG = np.array(hm.FLAG, np.uint8)


def frame(payload, with_crc=True, flip=None):
    """hdlc_model.frame_bits with one flag on either side, as an array; flip: a bit of the body (the checksum included) turned
    over before stuffing"""
    body = bytes(payload)
    if with_crc:
        c = hm.crc16_x25(body)
        body += bytes([c & 0xff, c >> 8])
    raw = bits_of(body).tolist()
    if flip is not None:
        raw[flip] ^= 1
    return np.array(hm.FLAG + hm.stuff(raw) + hm.FLAG, np.uint8)
