"""GPU: rr_hdlc_framer, rr_scrambler_g3ruh and rr_nrzi_encode (kernels_frame.hip) against the sequential chain of
tests/frame_model.py.  Every comparison is bit for bit: the blocks are exact in integers, so there is no tolerance anywhere in
this file.

The framer handles are module-scoped, one per flag set, and carry the scrambler's register and the NRZI level from test to test;
the Rig below keeps, per handle, the list of pushes it has seen and runs the sequential model from the state that list left, so
the expectation follows the handle whatever the order of the tests."""
import json
import os

import numpy as np
import pytest
import torch

import bits_model as bm
import frame_model as fm
import hdlc_model as hm
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "hdlc_framer_known_answers.json")))
LO, HI = -0.5, 2.0
ALL_FLAGS = list(range(16))
SLACK = 257                           # canary elements behind the bound


def launches():
    return rr.lib().rr_debug_kernel_launches()


def geometry(packets):
    lens = np.array([len(p) for p in packets], np.uintp)
    return b"".join(bytes(p) for p in packets), (np.cumsum(lens) - lens).astype(np.uintp), lens


def push_dev(fr, packets, geom=None):
    """one push through device buffers -> (out[:produced], records, produced); the elements behind `produced` keep their canary"""
    data, starts, lens = geometry(packets) if geom is None else geom
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    cap = fr.bound(lens)
    f32 = fr.out_dtype == np.float32
    canary = 777.0 if f32 else 0xA5
    d_out = torch.full((cap + SLACK,), canary, dtype=torch.float32 if f32 else torch.uint8, device="cuda")
    fr.push_dev(d_in.data_ptr(), len(data), starts, lens, d_out.data_ptr(), cap)
    recs, produced = fr.records()
    out = d_out.cpu().numpy()
    assert produced <= cap
    assert np.all(out[produced:] == canary), "elements at and beyond `produced` were written"
    return out[:produced], recs, produced


class Rig:
    def __init__(self):
        self.fr = {f: rr.HdlcFramer(f, LO, HI) for f in ALL_FLAGS}
        self.hist = {f: () for f in ALL_FLAGS}
        self.cache = {}               # (flags & 7, history) -> (bits, records, (shift_reg, level))

    def expect(self, flags, name, packets):
        f7, hist = flags & 7, self.hist[flags]
        key = (f7, hist + (name,))
        if key not in self.cache:
            m = fm.FramerSeq(f7)
            if hist:
                m.lfsr.shift_reg, m.level = self.cache[(f7, hist)][2]
            bits, recs = m.push(packets)
            bits.setflags(write=False)
            self.cache[key] = (bits, recs, (m.lfsr.shift_reg, m.level))
        bits, recs, _ = self.cache[key]
        self.hist[flags] = key[1]
        return (np.where(bits != 0, np.float32(HI), np.float32(LO)) if flags & fm.SYMBOLS else bits), recs

    def check(self, flags, name, packets):
        """one push of `packets` into the handle of `flags`: output, records and produced against the sequential model"""
        want, wrecs = self.expect(flags, name, packets)
        got, recs, produced = push_dev(self.fr[flags], packets)
        assert got.dtype == want.dtype and produced == len(want), (flags, name, produced, len(want))
        assert np.array_equal(got, want), (flags, name, int(np.argmax(got != want)))
        assert [(int(r["start"]), int(r["len"]), int(r["stuffed"]), int(r["fcs"])) for r in recs] == wrecs, (flags, name)
        return got


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def T(rig):
    t = rig.fr[0].tile_bits
    assert t % 64 == 0 and all(rig.fr[f].tile_bits == t for f in ALL_FLAGS)
    return t


# ---- 1. the reference's vectors ---------------------------------------------------------------------------------------------------
def test_vectors_through_every_block(rig):
    flag = VECTORS["sync"] * VECTORS["sync_bytes"]
    various = [bytes.fromhex(v["bytes"]) for v in VECTORS["various"]]
    for k, v in enumerate(VECTORS["various"]):                # each alone through the plain framer, against the vector itself
        got, recs, _ = push_dev(rig.fr[0], [various[k]])
        assert got.tolist() == flag + [int(c) for c in v["bits"]] + flag
    fcs = bytes.fromhex(VECTORS["fcs"]["bytes"])
    app = bytes.fromhex(VECTORS["fcs"]["appended"])
    got, recs, _ = push_dev(rig.fr[fm.FCS], [fcs])
    assert int(recs[0]["fcs"]) == app[0] | app[1] << 8
    assert np.array_equal(got, fm.FramerSeq(0).push([fcs + app])[0])
    for f in ALL_FLAGS:                                       # all of them as one batch through every flag set
        rig.check(f, "vectors", various + [fcs])
    for v in VECTORS["scrambler"]:
        y = rr.Scrambler.g3ruh().work(np.array(v["input"] + [0] * v["flush"], np.uint8), 100)[4]
        assert y[:17].tolist() == [0] * 17 and y[v["skip"]:].tolist() == v["scrambled"]
    enc = VECTORS["nrzi"][1]
    assert enc["block"] == "NrziEncode"
    assert rr.NrziEncode().work(np.array(enc["input"], np.uint8), 100)[4].tolist() == enc["output"]
    dec = VECTORS["nrzi"][0]                                  # NrziDecode's vector backwards: encode its output's source
    assert rr.NrziDecode().work(rr.NrziEncode().work(np.array(dec["input"], np.uint8), 100)[4], 100)[4].tolist() == dec["input"]


# ---- 2. seams ------------------------------------------------------------------------------------------------------------------------
def seam_payloads(T):
    tb = T // 8
    rng = np.random.default_rng(5)
    z = lambda n: b"\x00" * n
    out = {
        "all ones over three tiles": [b"\xff" * (3 * tb + 1)],
        # the payload ends one byte in front of a tile's end, at it, and one byte behind it; a second packet follows
        "payload ends around a tile": [z(tb - 1), b"\xff\x0f", z(tb - 2), b"\x7f", z(tb), b"\xf0" * 3, z(tb + 1), b"\x55"],
        # ... and the FRAME ends at T - 1, T and T + 1 bits of the line: 320 + 8 L + stuffed with 7, 8 and 9 stuffed bits
        "frame ends around a tile": [b"\x1f" * k + z((T - 320 - 8) // 8 - k) for k in (7, 8, 9)],
        "five ones end the packet": [z(3) + b"\xf8", b"\xf8", b"\x1f\xf8", b"\xff\xff\xc1\x07"],
        "five ones end the tile": [z(tb - 1) + b"\xf8" + b"\x01" + z(5), z(tb - 1) + b"\xf8" + b"\xfe"],
        "four ones end the tile, one begins the next": [z(tb - 1) + b"\xf0" + b"\x01" + z(9), z(tb - 1) + b"\xf0" + b"\xff\xff"],
        "3000 packets of 0 and 1 bytes": [bytes([int(v)]) if k else b"" for k, v in
                                         zip(rng.integers(0, 2, 3000), rng.choice([0xff, 0x1f, 0xf8, 0x00, 0x7e], 3000))],
    }
    return out


SEAMS = ["all ones over three tiles", "payload ends around a tile", "frame ends around a tile", "five ones end the packet",
         "five ones end the tile", "four ones end the tile, one begins the next", "3000 packets of 0 and 1 bytes"]


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("name", SEAMS)
def test_seams(rig, T, name, flags):
    packets = seam_payloads(T)[name]
    rig.check(flags, name, packets)
    if name == "all ones over three tiles" and not flags & fm.FCS:
        assert rig.fr[flags].records()[1] == rig.fr[flags].bound([len(packets[0])])      # the bound is reached
    if name == "frame ends around a tile" and flags == 0:
        assert [int(r["len"]) for r in rig.fr[0].records()[0]] == [T - 1, T, T + 1]


# ---- 3. the split into pushes --------------------------------------------------------------------------------------------------------
def test_split_invariance():
    rng = np.random.default_rng(6)
    packets = fm.draw_packets(rng, 40, 120)
    flags = fm.FCS | fm.G3RUH | fm.NRZI
    want = fm.FramerSeq(flags).push(packets)[0]

    def run(cuts):
        fr = rr.HdlcFramer(flags)
        return np.concatenate([push_dev(fr, packets[a:b])[0] for a, b in zip([0] + cuts, cuts + [len(packets)])])

    assert np.array_equal(run([]), want)
    assert np.array_equal(run(list(range(1, 40))), want)
    for _ in range(5):
        cuts = sorted(int(v) for v in rng.integers(0, 41, int(rng.integers(1, 8))))      # (equal cuts: pushes of no packets)
        assert np.array_equal(run(cuts), want), cuts


def test_the_scramblers_lag_of_17_bits_is_visible():
    rng = np.random.default_rng(7)
    a, b = fm.draw_packets(rng, 3, 50), fm.draw_packets(rng, 2, 50)
    plain_a, plain_b = fm.FramerSeq(0).push(a)[0], fm.FramerSeq(0).push(b)[0]
    fr = rr.HdlcFramer(fm.G3RUH)
    out_a = push_dev(fr, a)[0]
    out_b = push_dev(fr, b)[0]
    rx = bm.Lfsr(*bm.G3RUH)
    dec_a = np.array(rx.run(out_a), np.uint8)                 # Descrambler undoes the scrambler, 17 bits late
    assert len(out_a) == len(plain_a) and np.array_equal(dec_a[17:], plain_a[:-17])
    dec_b = np.array(rx.run(out_b), np.uint8)
    assert np.array_equal(dec_b[:17], plain_a[-17:])          # the last 17 bits of the first push come out with the next one
    assert np.array_equal(dec_b[17:], plain_b[:-17])


# ---- 4. fusion -----------------------------------------------------------------------------------------------------------------------
def test_fusion_equals_the_three_blocks_through_device_buffers():
    rng = np.random.default_rng(8)
    batches = [fm.draw_packets(rng, 30, 400), fm.draw_packets(rng, 7, 90)]
    fused, plain, scr, nrzi = rr.HdlcFramer(fm.G3RUH | fm.NRZI), rr.HdlcFramer(0), rr.Scrambler.g3ruh(), rr.NrziEncode()
    for packets in batches:
        want = push_dev(fused, packets)[0]
        data, starts, lens = geometry(packets)
        cap = plain.bound(lens)
        d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        d_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        plain.push_dev(d_in.data_ptr(), len(data), starts, lens, d_a.data_ptr(), cap)
        n = plain.records()[1]
        assert scr.work_dev(d_a.data_ptr(), n, d_b.data_ptr(), n)[1:3] == (n, n)
        assert nrzi.work_dev(d_b.data_ptr(), n, d_c.data_ptr(), n)[1:3] == (n, n)
        nrzi.sync()
        assert n == len(want) and np.array_equal(d_c.cpu().numpy()[:n], want)


@pytest.mark.parametrize("w", [1, 17, 18, 4097])
def test_sync_blocks_cut_into_windows(w):
    rng = np.random.default_rng(9)
    n = {1: 300, 17: 17 * 130, 18: 18 * 130, 4097: 3 * 4097 + 5}[w]
    x = (rng.random(n) < 0.7).astype(np.uint8) | (rng.integers(0, 128, n).astype(np.uint8) << 1)      # only the lowest bit is read
    for make, flags in ((rr.Scrambler.g3ruh, fm.G3RUH), (rr.NrziEncode, fm.NRZI)):
        want = np.array(fm.FramerSeq(flags).line(x & 1), np.uint8)
        blk = make()
        got = []
        for i in range(0, n, w):
            st, c, p, need, y = blk.work(x[i:i + w], w)
            assert c == p == len(x[i:i + w])
            got.append(y)
        assert np.array_equal(np.concatenate(got), want), (blk.name, w)
        assert np.array_equal(make().work(x, n)[4], want)     # and in one call


# ---- 5. symbols ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(8))
def test_symbols_are_the_bits_mapped(rig, f):
    packets = fm.draw_packets(np.random.default_rng(10), 25, 200)
    bits = rig.check(f, "symbols", packets)
    sym = rig.check(f | fm.SYMBOLS, "symbols", packets)
    if rig.hist[f] == rig.hist[f | fm.SYMBOLS]:               # the twins have seen the same stream: the same bits
        assert sym.dtype == np.float32 and np.array_equal(sym, np.where(bits != 0, np.float32(HI), np.float32(LO)))


# ---- 6. loop-back on the device -------------------------------------------------------------------------------------------------------
def test_loop_back_on_the_device():
    rng = np.random.default_rng(11)
    packets = [bytes(rng.integers(0, 256, int(rng.integers(20, 301)), dtype=np.uint8)) for _ in range(64)]
    fr = rr.HdlcFramer(fm.FCS | fm.G3RUH | fm.NRZI | fm.SYMBOLS, -1.0, 1.0)
    data, starts, lens = geometry(packets)
    cap = fr.bound(lens)
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_sym = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    fr.push_dev(d_in.data_ptr(), len(data), starts, lens, d_sym.data_ptr(), cap)
    n = fr.records()[1]
    rx = rr.BitDecoder(nrzi=True, descrambler=bm.G3RUH)
    assert rx.work_dev(d_sym.data_ptr(), n, d_bits.data_ptr(), n)[1:3] == (n, n)
    rx.sync()
    m = hm.HdlcModel(min_size=0, max_size=4096)
    got = [f[1] for f in m.run(d_bits.cpu().numpy()[:n])]
    assert got == packets and m.stats() == (64, 0, 0)


# ---- 7. fuzz -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(30))
def test_fuzz(rig, seed):
    rng = np.random.default_rng(1000 + seed)
    packets = fm.draw_packets(rng, int(rng.integers(1, 201)), 2000)
    rig.check([7, 15, 6, 3, 5, 1, 2, 4, 0, 14][seed % 10], f"fuzz{seed}", packets)


def test_beyond_one_chunk_of_the_two_scans(T):
    """more than 1024 tiles: the single-workgroup scans of the stuffing summaries and of the line coder's states go round their
    loop.  5 M bits cost the sequential model 8 s, so this one case is held to the closed form, which tests/test_frame_cpu.py
    holds to the sequential model."""
    rng = np.random.default_rng(13)
    n = 1030 * T // 8 + 77
    packets = [np.packbits((rng.random(8 * n) < 0.9).astype(np.uint8), bitorder="little").tobytes(), b"\xff" * (70 * T // 8 + 3), b"\x0f"]
    flags = fm.FCS | fm.G3RUH | fm.NRZI
    want, wrecs = fm.closed_form(packets, flags)
    fr = rr.HdlcFramer(flags)
    got, recs, produced = push_dev(fr, packets)
    assert produced == len(want) > 1100 * T and np.array_equal(got, want)
    assert [(int(r["start"]), int(r["len"]), int(r["stuffed"]), int(r["fcs"])) for r in recs] == wrecs
    # the state it leaves is the stream's: one more push continues the closed form of the whole
    more = [b"\xf8\x1f"]
    got2 = push_dev(fr, more)[0]
    assert np.array_equal(got2, fm.closed_form(packets + more, flags)[0][len(want):])


# ---- 8. launches, refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, fm.FCS, fm.SYMBOLS, fm.FCS | fm.G3RUH | fm.NRZI, 15])
def test_launch_count_does_not_depend_on_the_payload(rig, T, flags):
    sizes = [0, 1, T // 8, 3 * T // 8 + 1, 5, 700]
    counts = []
    for name, fill in (("zeros", b"\x00"), ("ones", b"\xff")):
        packets = [fill * n for n in sizes]
        want, _ = rig.expect(flags, f"launches {name}", packets)
        before = launches()
        got = push_dev(rig.fr[flags], packets)[0]
        counts.append(launches() - before)
        assert np.array_equal(got, want)
    assert counts[0] == counts[1] > 0
    assert counts[0] == 3 + (2 if flags & fm.FCS else 0) + (3 if flags & 6 else 1 if flags & fm.SYMBOLS else 0)


def test_refusals_launch_nothing(rig):
    fr = rig.fr[fm.FCS | fm.G3RUH]
    packets = [b"\xff" * 10, b"\x00" * 3]
    data, starts, lens = geometry(packets)
    cap = fr.bound(lens)
    assert cap == sum(320 + 8 * (n + 2) + 8 * (n + 2) // 5 for n in (10, 3))
    d_in = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_out = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    before = launches()
    with pytest.raises(RuntimeError, match="output shorter than the framed bits can be"):
        fr.push_dev(d_in.data_ptr(), len(data), starts, lens, d_out.data_ptr(), cap - 1)
    with pytest.raises(RuntimeError, match="packet outside the buffer"):
        fr.push_dev(d_in.data_ptr(), len(data) - 1, starts, lens, d_out.data_ptr(), cap)
    with pytest.raises(RuntimeError, match="packet outside the buffer"):
        fr.push_dev(d_in.data_ptr(), len(data), [len(data) + 1], [0], d_out.data_ptr(), cap)
    with pytest.raises(RuntimeError, match="2\\^30"):        # a bound above 2^30 elements (nothing of the buffer is touched)
        fr.push_dev(d_in.data_ptr(), 1 << 28, [0], [1 << 27], d_out.data_ptr(), 1 << 40)
    with pytest.raises(RuntimeError, match="rr_hdlc_framer_push"):
        fr.work(np.zeros(8, np.uint8), 8)
    with pytest.raises(ValueError, match="unknown hdlc framer flags"):
        rr.HdlcFramer(16)
    # no packets: nothing launched, no records, the state left alone
    fr.push_dev(d_in.data_ptr(), len(data), [], [], d_out.data_ptr(), 0)
    recs, produced = fr.records()
    assert len(recs) == 0 and produced == 0
    assert launches() == before
    assert np.all(d_out.cpu().numpy() == 0xA5)
    # overlapping and repeated ranges are read-only input: fine; and the handle's state is still the model's
    rig.check(fm.FCS | fm.G3RUH, "after the refusals", packets)
    want, wrecs = rig.expect(fm.FCS | fm.G3RUH, "overlap", [data[0:13], data[0:13], data[5:9]])
    got, recs, _ = push_dev(fr, None, geom=(data, np.array([0, 0, 5], np.uintp), np.array([13, 13, 4], np.uintp)))
    assert np.array_equal(got, want) and [int(r["fcs"]) for r in recs] == [r[3] for r in wrecs]


def test_host_push_equals_device_push(rig):
    packets = fm.draw_packets(np.random.default_rng(12), 9, 300)
    for flags in (0, 7, 15):
        want, wrecs = rig.expect(flags, "host push", packets)
        got = rig.fr[flags].push(packets)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        recs, produced = rig.fr[flags].records()
        assert produced == len(want) and [int(r["stuffed"]) for r in recs] == [r[2] for r in wrecs]
