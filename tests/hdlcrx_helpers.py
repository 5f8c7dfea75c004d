"""What the rr.HdlcReceiver tests share: the per-stream oracle made of the project's Python machines (bits_model.Chain feeding
hdlc_model.HdlcModel), line coding of drawn HDLC streams into soft symbols, and the input of the SymbolSync -> HdlcReceiver chain
test, whose end-to-end condition tests/test_hdlcrx_cpu.py asserts on the models."""
import numpy as np

import bits_model as bm
import hdlc_model as hm
import symsync_model as sm

G3RUH = (0x21, 0, 16)
# name -> (invert, nrzi, descrambler)
LINE_CONFIGS = {"plain": (False, False, None), "nrzi": (False, True, None), "nrzi+g3ruh": (False, True, G3RUH),
                "invert+nrzi+g3ruh": (True, True, G3RUH)}


class ModelReceiver:
    """one stream of rr.HdlcReceiver: Chain (no correlator) -> HdlcModel, state carried from push to push"""

    def __init__(self, min_size, max_size, invert=False, nrzi=False, descrambler=None, flags=0):
        self.chain = bm.Chain(invert=invert, nrzi=nrzi, descrambler=descrambler)
        self.hdlc = hm.HdlcModel(min_size, max_size, bool(flags & 1), bool(flags & 2))

    def push(self, syms):
        """-> [(pos, bytes, fixed)] of the frames that ended inside these symbols"""
        if len(syms) == 0:
            return []
        return self.hdlc.run(self.chain.run(np.asarray(syms, np.float32))[0].tolist())

    def stats(self):
        return tuple(self.hdlc.stats())


def line_encode(bits, invert=False, nrzi=False, descrambler=None):
    """HDLC bits -> soft symbols that the chain (invert, nrzi, descrambler) decodes back to them: [Scrambler] -> [NrziEncode] ->
    [XorConst(1)] -> +-1.  Scrambler (descrambler.rs:41-47) hands out its register's OLDEST bit, so behind it the stream is
    length + 1 bits late and its last length + 1 bits stay in the register: end the bits with that many to spare."""
    b = [int(v) for v in bits]
    if descrambler is not None:
        b = bm.scramble(b, *descrambler)
    if nrzi:
        b = bm.nrzi_encode(b)
    a = np.array(b, np.int64)
    if invert:
        a = 1 - a
    return (2.0 * a - 1.0).astype(np.float32)


# ---- the chain test: SymbolSync(4.0, 0.0, [0.0001, 0.99999999], N) -> HdlcReceiver(G3RUH, NRZI) --------------------------------------
CHAIN_N, CHAIN_SPS, CHAIN_TAPS, CHAIN_MAX_SIZE = 5, 4.0, [0.0001, 0.99999999], 60
CHAIN_CUT = 1200            # samples of the first of the two pushes: symbol 300, inside every stream's first frame


def chain_payloads(c, seed=77):
    rng = np.random.default_rng(seed + c)
    return [rng.integers(0, 256, 12 + 7 * c, dtype=np.uint8).tobytes() for _ in range(3)]


def chain_samples():
    """-> f32[CHAIN_N, n]: per stream 20 flags, then three frames of 12 + 7 c random bytes between 2 + c flags (and 4 more flags
    for the scrambler to push the last frame out), G3RUH-scrambled, NRZI-encoded and held over 4 samples a symbol; the shorter
    streams end in their last level"""
    rows = []
    for c in range(CHAIN_N):
        bits = hm.FLAG * 20
        for p in chain_payloads(c):
            bits = bits + hm.frame_bits(p, 2 + c, 2 + c)
        rows.append(sm.hold(line_encode(bits + hm.FLAG * 4, nrzi=True, descrambler=G3RUH), CHAIN_SPS, 0.0))
    n = max(len(r) for r in rows)
    return np.stack([np.concatenate([r, np.full(n - len(r), r[-1], np.float32)]) for r in rows])


def chain_model(x, cuts):
    """the models over x in the pushes `cuts` (sample counts) -> (per push, per stream: symbols f32[]; per push, per stream: frames;
    per stream: stats)"""
    syncs = [sm.SymbolSync(CHAIN_SPS, 0.0, CHAIN_TAPS) for _ in range(len(x))]
    rxs = [ModelReceiver(1, CHAIN_MAX_SIZE, nrzi=True, descrambler=G3RUH) for _ in range(len(x))]
    syms, frames, at = [], [], 0
    for n in cuts:
        s = [syncs[c].run(x[c, at:at + n])[0] for c in range(len(x))]
        syms.append(s)
        frames.append([rxs[c].push(s[c]) for c in range(len(x))])
        at += n
    return syms, frames, [r.stats() for r in rxs]
