"""GPU: rr_hdlc_deframer (kernels_hdlc.hip) against the sequential machine of tests/hdlc_model.py.  Every comparison is bit for
bit: frames, positions, repaired flags and the three counters; there is no tolerance anywhere in this file.

The handles are module-scoped, one per configuration of CONFIGS, each paired with an HdlcModel that is fed the same bits, so
the expectation follows the handle whatever the order of the tests.  Between tests Rig.reset returns the model to Unsynced(0xff),
and Rig.clear, where a test aims at the tiles, the handle to its 8 halo bits as well.  No test creates handles in a loop."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import frame_model as fm
import hdlc_model as hm
import rustradio_amd as rr
from hdlc_model import FLAG, bytes_to_bits, crc16_x25, frame_bits, stuff
from hdlc_rig import Rig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "hdlc_known_answers.json")))
KEEP, FIX = rr.HDLC_KEEP_CHECKSUM, rr.HDLC_FIX_BITS
CONFIGS = [(0, 3, KEEP), (1, 1, KEEP), (1, 10, KEEP), (3, 10, KEEP), (1, 10, 0), (1, 10, FIX), (10, 1500, FIX), (0, 4096, 0)]


def launches():
    return rr.lib().rr_debug_kernel_launches()


class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


@pytest.fixture(scope="module")
def rig():
    return Rig(CONFIGS)


@pytest.fixture(scope="module")
def T(rig):
    t, c = rig.dev[(1, 10, KEEP)].dims()
    assert t % 64 == 0 and c == 81 + 16 + 16
    assert rig.dev[(0, 3, KEEP)].dims() == (t, 25 + 4 + 16) and rig.dev[(10, 1500, FIX)].dims() == (t, 12001 + 2400 + 16)
    return t


# ---- 1. the reference's vectors ---------------------------------------------------------------------------------------------------
def test_golden_vectors(rig):
    seen = 0
    for case in GOLDEN["cases"]:
        cfg = (case["min_size"], case["max_size"], KEEP if case["keep_checksum"] else 0)
        assert cfg in CONFIGS, cfg
        for s in case["bits"]:
            bits = [int(c) for c in s]
            for via in ("push", "dev"):
                rig.reset(cfg)
                got = rig.feed(cfg, bits, via)
                assert [f[1] for f in got] == [bytes(f) for f in case["frames"]], (case["name"], via)
            rig.reset(cfg)                          # one bit per push: the state is carried
            got = sum((rig.feed(cfg, [b]) for b in bits), [])
            assert [f[1] for f in got] == [bytes(f) for f in case["frames"]], case["name"]
            seen += len(got)
    assert seen > 5


# ---- 2. the quirks, each by name ----------------------------------------------------------------------------------------------------
def test_a_frame_of_exactly_max_size_bytes_is_dropped(rig):
    for cfg in ((0, 3, KEEP), (1, 10, KEEP)):
        for nbytes, delivered in ((cfg[1] - 1, True), (cfg[1], False)):
            payload = bytes(range(1, nbytes + 1))
            rig.reset(cfg)
            got = rig.feed(cfg, frame_bits(payload, with_crc=False))
            assert [f[1] for f in got] == ([payload] if delivered else []), (cfg, nbytes)


def test_after_two_flags_sharing_a_zero_a_third_sharing_again_stays_unsynced(rig):
    cfg = (1, 10, KEEP)
    body = stuff(bytes_to_bits(b"\x42")) + FLAG
    found = {}
    for k in (1, 2, 3, 4, 5):
        rig.reset(cfg)
        found[k] = [f[1] for f in rig.feed(cfg, FLAG[:7] * k + [0] + body, "dev")]
    assert found == {1: [b"\x42"], 2: [], 3: [], 4: [b"\x42"], 5: []}


def test_the_empty_frame(rig):
    rig.reset((0, 3, KEEP))
    got = rig.feed((0, 3, KEEP), FLAG + FLAG)
    assert [(f[1], f[2]) for f in got] == [(b"", False)] and got[0][0] == rig.model[(0, 3, KEEP)].pos - 1
    for cfg in ((0, 4096, 0), (1, 10, KEEP)):       # fewer than 2 bytes without keep_checksum, or fewer than min_size: nothing, no counter
        rig.reset(cfg)
        before = rig.dev[cfg].stats()
        assert rig.feed(cfg, FLAG + FLAG) == [] and rig.dev[cfg].stats() == before


def test_a_flip_in_the_crc_field_raises_both_counters_and_emits_nothing(rig):
    payload = b"hello"
    c = crc16_x25(payload) ^ 0x0400
    bits = FLAG + stuff(bytes_to_bits(payload + bytes([c & 0xff, c >> 8]))) + FLAG
    for cfg, delta in (((1, 10, FIX), (0, 1, 1)), ((1, 10, 0), (0, 1, 0))):
        rig.reset(cfg)
        before = rig.dev[cfg].stats()
        assert rig.feed(cfg, bits) == []
        assert tuple(a - b for a, b in zip(rig.dev[cfg].stats(), before)) == delta


def test_single_bit_repair_takes_the_lowest_byte_and_bit(rig):
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
    raw = bytes_to_bits(payload + bytes([crc16_x25(payload) & 0xff, crc16_x25(payload) >> 8]))
    for k in (0, 77, 8 * 24 - 1):
        broken = list(raw)
        broken[k] ^= 1
        bits = FLAG + stuff(broken) + FLAG
        rig.reset((10, 1500, FIX))
        before = rig.dev[(10, 1500, FIX)].stats()
        got = rig.feed((10, 1500, FIX), bits, "dev")
        assert [(f[1], f[2]) for f in got] == [(payload, True)], k
        assert tuple(a - b for a, b in zip(rig.dev[(10, 1500, FIX)].stats(), before)) == (1, 0, 1)
        rig.reset((0, 4096, 0))
        before = rig.dev[(0, 4096, 0)].stats()
        assert rig.feed((0, 4096, 0), bits) == []
        assert tuple(a - b for a, b in zip(rig.dev[(0, 4096, 0)].stats(), before)) == (0, 1, 0)


@pytest.mark.parametrize("cfg", [(0, 3, KEEP), (1, 10, KEEP)], ids=["max3", "max10"])
def test_an_overlong_reset_inside_the_last_7_bits_hides_the_flag(rig, cfg):
    """the family of tests/test_hdlc_cpu.py, each stream also cut into two pushes at every bit position"""
    behind = stuff(bytes_to_bits(b"\x15")) + FLAG
    for extra, hidden in ((-7, False), (-6, False), (-5, True), (1, True), (2, False)):
        bits = FLAG + [0] * (8 * cfg[1] + extra) + FLAG + behind
        assert len(bits) == 32 + 8 * cfg[1] + extra                    # 57 and 113 bits at extra == 1
        for cut in [None] + list(range(1, len(bits))):
            rig.reset(cfg)
            got = rig.feed(cfg, bits) if cut is None else rig.feed(cfg, bits[:cut]) + rig.feed(cfg, bits[cut:])
            assert (b"\x15" not in [f[1] for f in got]) == hidden, (cfg, extra, cut)


# ---- 3. a drawn stream in random windows ------------------------------------------------------------------------------------------------
DRAWN = {(0, 3, KEEP): (3464, None), (1, 10, KEEP): (1728, None), (1, 10, 0): (651, (651, 907, 0)), (1, 10, FIX): (790, (790, 768, 262))}


@pytest.fixture(scope="module")
def drawn():
    bits = hm.draw_stream(np.random.default_rng(11), 200000)
    bits.setflags(write=False)
    return bits


@pytest.mark.parametrize("cfg", list(DRAWN), ids=lambda c: "%d-%d-%d" % c)
def test_drawn_stream_in_random_windows(rig, drawn, cfg):
    rng = np.random.default_rng(12)
    rig.reset(cfg)
    before = rig.dev[cfg].stats()
    frames, at = [], 0
    while at < len(drawn):
        n = int(rng.integers(1, 5001))
        frames += rig.feed(cfg, drawn[at:at + n], "dev" if (at // 7) & 1 else "push")
        at += n
    nframes, stats = DRAWN[cfg]
    assert len(frames) == nframes
    delta = tuple(a - b for a, b in zip(rig.dev[cfg].stats(), before))
    assert delta[0] == nframes
    if stats is not None:
        assert delta == stats
    if cfg[2] & FIX:
        assert sum(f[2] for f in frames) == 139        # data repairs; the other fixes were flips in the CRC field


# ---- 4. long frames -------------------------------------------------------------------------------------------------------------------
def test_long_frames(rig):
    rng = np.random.default_rng(13)
    for cfg in ((10, 1500, FIX),):
        rig.reset(cfg)
        for n in (10, 255, 256, 1497, 1498, 1499):
            for payload in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), b"\xff" * n):
                got = rig.feed(cfg, frame_bits(payload), "dev")
                # with its two checksum bytes 1498 is exactly max_size: dropped, as the model drops it, and 1499 beyond
                assert [f[1] for f in got] == ([payload] if n + 2 < 1500 else []), n
    # one flipped data bit, low in the frame and in its last byte
    for n, k in ((1497, 77), (255, 8 * 255 - 3)):
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        raw = bytes_to_bits(payload + bytes([crc16_x25(payload) & 0xff, crc16_x25(payload) >> 8]))
        raw[k] ^= 1
        got = rig.feed((10, 1500, FIX), FLAG + stuff(raw) + FLAG, "dev")
        assert [(f[1], f[2]) for f in got] == [(payload, True)]
        assert rig.feed((0, 4096, 0), FLAG + stuff(raw) + FLAG) == []
    # three frames back to back in one window: a shared flag, then an unshared one
    p = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 12, 1000)]
    window = frame_bits(p[0], 1, 1) + frame_bits(p[1], 0, 1) + frame_bits(p[2], 1, 1)
    for cfg in ((0, 4096, 0), (10, 1500, FIX)):
        assert [f[1] for f in rig.feed(cfg, window, "dev")] == p


# ---- 5. tile seams ------------------------------------------------------------------------------------------------------------------------
def test_closing_flag_at_the_tile_seams(rig, T):
    """behind clear() a handle carries 8 bits, so bit i of the push is virtual bit i + 8 of the tiles"""
    cfg = (1, 10, KEEP)
    frame = frame_bits(b"\x42\x99\x10", with_crc=False)
    for off in (0, 1, 6, 7, T - 1):
        end = T + off - 8                           # the push bit that is the closing flag's last
        rig.clear(cfg)
        bits = [0] * (end + 1 - len(frame)) + frame + [0] * 9
        got = rig.feed(cfg, bits, "dev")
        assert [f[1] for f in got] == [b"\x42\x99\x10"] and got[0][0] == rig.model[cfg].pos - 10, off


def test_stuffed_zero_and_abort_across_a_seam(rig, T):
    cfg = (10, 1500, FIX)
    payload = b"\xff" * 700                         # a stuffed 0 behind every five bits: one alignment of six puts one on the seam's first bit
    for lead in range(6):
        rig.clear(cfg)
        assert [f[1] for f in rig.feed(cfg, [0] * lead + frame_bits(payload), "dev")] == [payload]
    cfg = (1, 10, KEEP)
    for k in range(1, 8):                           # seven ones, k of them in front of the seam, inside a frame
        rig.clear(cfg)
        head = FLAG + stuff(bytes_to_bits(b"\x01\x02"))
        bits = [0] * (T - 8 - k - len(head)) + head + [1] * 7 + [0] + frame_bits(b"\x33", with_crc=False)
        assert [f[1] for f in rig.feed(cfg, bits, "dev")] == [b"\x33"], k


def test_a_frame_spanning_three_tiles_and_pushes_of_a_tile(rig, T, drawn):
    cfg = (10, 1500, FIX)
    payload = np.random.default_rng(14).integers(0, 256, 1400, dtype=np.uint8).tobytes()
    rig.clear(cfg)
    bits = [0] * (T - 500) + frame_bits(payload)
    assert len(bits) > 3 * T - 500
    assert [f[1] for f in rig.feed(cfg, bits, "dev")] == [payload]
    cfg = (1, 10, KEEP)
    rig.clear(cfg)
    at, total = 0, 0
    for n in (T, T - 1, T + 1, T - 8, T):
        total += len(rig.feed(cfg, drawn[at:at + n], "dev"))
        at += n
    assert total > 50


# ---- 6. the loop-back on the device ------------------------------------------------------------------------------------------------------
def test_loop_back_on_the_device(rig):
    """packets -> rr_hdlc_framer(FCS | G3RUH | NRZI | SYMBOLS) -> rr_bit_decoder(NRZI | DESCRAMBLE, 0x21, 0, 16) -> the deframer, device
    buffer to device buffer; the descrambler's register holds the last 17 bits back, which are closing flags"""
    cfg = (0, 4096, 0)
    rng = np.random.default_rng(23)
    packets = [p for p in fm.draw_packets(rng, 40, 60) if len(p)]
    data = np.frombuffer(b"".join(packets), np.uint8).copy()
    lens = np.array([len(p) for p in packets], np.uintp)
    starts = (np.cumsum(lens) - lens).astype(np.uintp)
    fr = rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
    dec = rr.BitDecoder(nrzi=True, descrambler=(0x21, 0, 16))
    cap = fr.bound(lens)
    d_in = torch.from_numpy(data).cuda()
    d_sym = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    fr.push_dev(d_in.data_ptr(), len(data), starts, lens, d_sym.data_ptr(), cap)
    _, produced = fr.records()
    st, consumed, made, need = dec.work_dev(d_sym.data_ptr(), produced, d_bits.data_ptr(), cap)
    assert consumed == produced == made
    rig.reset(cfg)
    before = rig.dev[cfg].stats()
    got = rig.feed(cfg, d_bits[:made].cpu().numpy())                 # (the model's copy of the bits; the handle gets the device buffer below)
    assert [f[1] for f in got] == packets and all(not f[2] for f in got)
    assert tuple(a - b for a, b in zip(rig.dev[cfg].stats(), before)) == (len(packets), 0, 0)
    # ... and with nothing downloaded between the blocks
    rig.reset(cfg)
    want = rig.model[cfg].run(d_bits[:made].cpu().numpy())
    rig.dev[cfg].push_dev(d_bits.data_ptr(), made)
    assert rig.dev[cfg].result() == want and [f[1] for f in want] == packets
    assert rig.dev[cfg].stats() == rig.model[cfg].stats()


# ---- 7. bounds and canaries ---------------------------------------------------------------------------------------------------------------
def test_fetches_respect_cap_and_the_arena_is_the_device_arena(rig):
    cfg = (1, 10, KEEP)
    rig.reset(cfg)
    bits = sum((frame_bits(bytes([k + 1] * (k + 1)), with_crc=False) for k in range(6)), [])
    got = rig.feed(cfg, bits)
    assert len(got) == 6
    d, L = rig.dev[cfg], rr.lib()
    rec = d.frames()
    arena = d.frame_bytes()
    total = C.c_size_t(0)
    for cap in (0, 1, len(rec)):
        buf = np.zeros(cap + 3, rr.HDLC_FRAME)
        buf.view(np.uint8)[:] = 0xA5
        assert L.rr_hdlc_frames(d._h, buf.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(total)) == 0
        assert total.value == len(rec) and np.array_equal(buf[:cap], rec[:cap]) and np.all(buf[cap:].view(np.uint8) == 0xA5)
    for cap in (0, 1, len(arena)):
        out = np.full(cap + 3, 0xA5, np.uint8)
        assert L.rr_hdlc_frame_bytes(d._h, out.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(total)) == 0
        assert total.value == len(arena) and np.array_equal(out[:cap], arena[:cap]) and np.all(out[cap:] == 0xA5)
    p, n = d.bytes_dev()
    assert p and n == len(arena)
    assert np.array_equal(torch.as_tensor(_DevMem(p, n), device="cuda").cpu().numpy(), arena)
    for r in rec:
        assert int(r["start"]) + int(r["len"]) <= n and int(r["len"]) <= 10
    assert int(np.count_nonzero(arena)) == sum(len(f[1]) for f in got)         # bytes of no frame are 0


def test_launch_count_depends_on_the_length_alone(rig):
    cfg = (1, 10, KEEP)
    n = 3 * 4096 + 17
    counts = []
    for bits in (np.zeros(n, np.uint8), np.resize(np.array(FLAG[:7], np.uint8), n), np.resize(np.array(FLAG, np.uint8), n),
                 np.ones(n, np.uint8)):
        rig.reset(cfg)
        t = torch.from_numpy(bits).cuda()
        m = rig.model[cfg].run(bits)
        before = launches()
        rig.dev[cfg].push_dev(t.data_ptr(), n)
        counts.append(launches() - before)
        assert rig.dev[cfg].result() == m
    assert len(set(counts)) == 1 and counts[0] == 7, counts


def test_an_empty_push_changes_nothing(rig):
    cfg = (1, 10, KEEP)
    rig.reset(cfg)
    half = frame_bits(b"\x42\x43", with_crc=False)
    assert rig.feed(cfg, half[:20]) == []
    stats = rig.dev[cfg].stats()
    before = launches()
    assert rig.feed(cfg, []) == [] and rig.feed(cfg, [], "dev") == []
    assert launches() == before and rig.dev[cfg].stats() == stats
    assert rig.dev[cfg].bytes_dev() == (None, 0) and len(rig.dev[cfg].frame_bytes()) == 0
    assert [f[1] for f in rig.feed(cfg, half[20:])] == [b"\x42\x43"]


def test_a_handle_may_go_after_push_dev_without_a_fetch():
    d = rr.HdlcDeframer(1, 10, FIX)
    t = torch.from_numpy(np.array(frame_bits(b"abc") * 3, np.uint8)).cuda()
    d.push_dev(t.data_ptr(), len(t))
    del d
    torch.cuda.synchronize()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rig):
    with pytest.raises(ValueError, match="unknown hdlc deframer flags"):
        rr.HdlcDeframer(1, 10, 4)
    with pytest.raises(ValueError, match="hdlc deframer: max_size beyond 65535"):
        rr.HdlcDeframer(1, 65536)
    d = rig.dev[(1, 10, KEEP)]
    rig.reset((1, 10, KEEP))
    stats = d.stats()
    before = launches()
    with pytest.raises(ValueError, match="hdlc deframer: more than 2\\^30 bits in one push"):
        d.push_dev(1 << 20, (1 << 30) + 1)
    with pytest.raises(ValueError, match="hdlc deframer: null bits"):
        d.push_dev(0, 5)
    assert rr.lib().rr_hdlc_deframer_push(d._h, None, 3) != 0 and rr.last_error() == "hdlc deframer: null bits"
    assert launches() == before and d.stats() == stats
    t = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="HdlcDeframer delivers frames"):
        d.work_dev(t.data_ptr(), 8, t.data_ptr() + 8, 8)
    assert rr.lib().rr_hdlc_frames(rr.HdlcFramer(0)._h, None, 0, C.byref(C.c_size_t(0))) != 0
    assert "not an hdlc deframer handle" in rr.last_error()
    assert [f[1] for f in rig.feed((1, 10, KEEP), frame_bits(b"\x07", with_crc=False))] == [b"\x07"]       # the handle is as it was
