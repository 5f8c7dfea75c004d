"""GPU: rr_hdlc_deframer (kernels_hdlc.hip) where only a device goes: gaps of thousands of bits carried from push to push, more
than one chunk of the two single-workgroup scans, more than one pass of every grid-stride loop, the lane and segment partition
of the emitting wave, a full record list, bodies past the CRC's period, and pushes that nobody fetched.

As in tests/test_gpu_hdlc.py every comparison is bit for bit against the sequential machine of tests/hdlc_model.py — frames
(pos, bytes, fixed) and the three counters, inside Rig.feed — the handles are module-scoped, one per configuration, and
Rig.clear between tests returns handle and model to Unsynced(0xff) with 8 bits carried.  The models repair with find_right_crc_lockstep
(tests/test_hdlc_cpu.py holds it to find_right_crc), memoised: the same broken frame comes back cut at many places.

Every test first shows ON THE HOST, from its own input, dims() and the device's CU count, that the loop it is aimed at is
entered, and fails if it is not: a test that no longer reaches its loop must not go on passing."""
import functools

import numpy as np
import pytest
import torch

import hdlc_model as hm
from hdlc_rig import FIX, FLAG, HALO, KEEP, Rig, carried_at_least, flag_ends, frame, reach, stuffed_ones, to_dev

pytestmark = pytest.mark.gpu
CONFIGS = [(0, 3, KEEP), (1, 10, KEEP), (1, 10, FIX), (10, 1500, FIX), (0, 4096, 0), (0, 65535, FIX), (0, 65535, KEEP)]
CARRY_STEP = 256        # threads of k_hdlc_carry: its copy loop steps by this
SCAN = 1024             # tiles (k_hdlc_offs) and gap blocks (k_hdlc_resolve) of one chunk of the single-workgroup scans
GAP_BLOCK = 256         # gaps of one block of k_hdlc_gap
GROUPS_PER_CU = 8       # the grid-stride kernels launch at most this many workgroups per CU; k_hdlc_emit's hold 4 waves


@pytest.fixture(scope="module")
def rig():
    return Rig(CONFIGS, functools.lru_cache(maxsize=None)(hm.find_right_crc_lockstep))


@pytest.fixture(scope="module")
def T(rig):
    t, c = rig.dev[(10, 1500, FIX)].dims()
    assert t % 64 == 0 and c == HALO + reach(1500) and rig.dev[(0, 65535, KEEP)].dims() == (t, HALO + reach(65535))
    return t


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def drawn():
    bits = hm.draw_stream(np.random.default_rng(11), 200000)
    bits.setflags(write=False)
    return bits


class Feed:
    """pushes behind a clear(): bit i of the first is virtual bit 8 + i; carried[i] is a lower bound of what push i found on the
    device, and exact while the model collects"""

    def __init__(self, rig, cfg):
        rig.clear(cfg)
        self.rig, self.cfg, self.seen, self.carried = rig, cfg, np.zeros(0, np.uint8), [HALO]

    def push(self, bits, via="dev"):
        got = self.rig.feed(self.cfg, bits, via)
        self.seen = np.concatenate([self.seen, np.asarray(bits, np.uint8)])
        self.carried.append(carried_at_least(self.seen, self.rig.model[self.cfg]))
        return got


def delta(rig, cfg, before):
    return tuple(a - b for a, b in zip(rig.dev[cfg].stats(), before))


def flipped(data, h):
    out = bytearray(data)
    out[h >> 3] ^= 1 << (h & 7)
    return bytes(out)


# ---- 1. long gaps carried across pushes ------------------------------------------------------------------------------------------------
LONG = (10, 1500, FIX)


@pytest.fixture(scope="module")
def long_frames():
    """name -> (bits, the payload delivered, repaired)"""
    rng = np.random.default_rng(41)
    out = {}
    for name, payload, h in (("random", rng.integers(0, 256, 1497, dtype=np.uint8).tobytes(), 77), ("ones", b"\xff" * 1497, 8 * 31 + 2)):
        out[name] = (frame(payload), payload, False)
        out[name + "-flipped"] = (frame(payload, flip=h), payload, True)       # an early bit: the repair reads bytes of earlier pushes
    return out


VARIANTS = ["random", "random-flipped", "ones", "ones-flipped"]


@pytest.mark.parametrize("name", VARIANTS)
def test_a_long_frame_cut_in_two_at_the_carry_steps_and_tile_seams(rig, T, long_frames, name):
    """k_hdlc_carry's copy loop beyond its first step, hd_bit reading cin beyond the first tile, the gap thread and the emitting
    wave reading words that were carried.  Behind clear() a first push of c >= 8 bits of the frame leaves exactly c carried."""
    bits, payload, fixed = long_frames[name]
    L, cap = len(bits), rig.dev[LONG].dims()[1]
    seams = [CARRY_STEP, 2 * CARRY_STEP] + [k * T for k in range(1, (L - 2) // T + 1)]
    cuts = set(range(1, 17)) | set(range(L - 16, L)) | {b + d for b in seams for d in (-1, 0, 1)}
    found = set()
    for c in sorted(cuts):
        f = Feed(rig, LONG)
        got = f.push(bits[:c]) + f.push(bits[c:], "push" if c & 1 else "dev")
        assert [(x[1], x[2]) for x in got] == [(payload, fixed)], (name, c)
        assert f.carried[1] == (c if c >= 8 else HALO)
        found.add(f.carried[1])
    for b in seams:
        assert {b - 1, b, b + 1} <= found, b
    assert max(found) == L - 1 and 2 * T < L - 1 <= cap and T > 2 * CARRY_STEP
    if name.startswith("ones"):
        assert L - 1 > 3 * T and cap - L < 64              # three seams of the virtual stream, and the carry all but full


@pytest.mark.parametrize("name", VARIANTS)
def test_a_long_frame_in_random_pieces_and_bit_by_bit_at_its_end(rig, T, long_frames, name):
    bits, payload, fixed = long_frames[name]
    rng = np.random.default_rng(42)
    f, got, at = Feed(rig, LONG), [], 0
    while at < len(bits):
        n = int(rng.integers(1, 701))
        got += f.push(bits[at:at + n], "dev" if at & 1 else "push")
        at += n
    assert [(x[1], x[2]) for x in got] == [(payload, fixed)]
    assert sum(c > CARRY_STEP for c in f.carried[:-1]) > 10 and sum(c > 2 * T for c in f.carried[:-1]) >= 2
    f = Feed(rig, LONG)
    got = f.push(bits[:-64])
    for b in bits[-64:]:
        got += f.push([b], "push")
    assert [(x[1], x[2]) for x in got] == [(payload, fixed)]
    assert len(f.carried) == 66 and min(f.carried[1:65]) > 2 * T


def _open_gap(first):
    """the bits behind the last flag end of a first push"""
    return len(first) - 1 - int(flag_ends(first)[-1])


def _open_gap_stream(kind, g, tail):
    gap = np.zeros(g, np.uint8) if kind == "zeros" else stuffed_ones(g)
    x = np.concatenate([FLAG, gap, tail])
    assert list(flag_ends(x[:HALO + g + 7])) == [7]        # up to the closing flag's seventh bit the only flag end is the first
    return x


@pytest.mark.parametrize("kind", ["zeros", "ones"])
def test_an_open_gap_grows_past_reach_while_it_is_carried(rig, T, kind):
    """hdlc_carry_plan's second reason to cut the carry down to the halo, at a max_size where the gap spans tiles.  The first
    flag ends at bit 7 in state S (from U every gap leads to S), so a first push of 8 + k bits leaves an open gap of k."""
    R = reach(1500)
    assert R > 3 * T
    payload = bytes(range(40, 52))
    tail, opens = frame(payload), set()
    for g in range(R - 2, R + 4):
        x = _open_gap_stream(kind, g, tail)
        for k in (None, R - 1, R, R + 1, R + 2):
            f = Feed(rig, LONG)
            if k is None:
                got = f.push(x)
            else:
                assert _open_gap(x[:HALO + k]) == k and k < g + 8          # (the cut lies in front of the closing flag's end)
                got = f.push(x[:HALO + k]) + f.push(x[HALO + k:])
                opens.add(k - R)
            assert [(y[1], y[2]) for y in got] == [(payload, False)], (kind, g, k)
    assert opens == {-1, 0, 1, 2}                          # carried whole up to reach, cut down to the halo beyond it


def test_an_open_gap_grows_past_reach_at_the_largest_max_size(rig, T):
    cfg = (0, 65535, KEEP)
    R = reach(65535)
    assert rig.dev[cfg].dims()[1] == HALO + R == 629153
    tail = frame(b"\x42\x43", with_crc=False)
    x = _open_gap_stream("ones", R + 3, tail)
    for k in (R - 1, R, R + 1, R + 2):
        f = Feed(rig, cfg)
        assert _open_gap(x[:HALO + k]) == k
        got = f.push(x[:HALO + k]) + f.push(x[HALO + k:])
        assert [y[1] for y in got] == [b"\x42\x43"], k


def test_the_longest_frame_whole_and_in_three_pushes(rig, T):
    cfg = (0, 65535, KEEP)
    payload = np.random.default_rng(43).integers(0, 256, 65534, dtype=np.uint8).tobytes()
    x = frame(payload, with_crc=False)
    f = Feed(rig, cfg)
    assert [y[1] for y in f.push(x)] == [payload]
    f = Feed(rig, cfg)
    got = f.push(x[:200001]) + f.push(x[200001:400003]) + f.push(x[400003:])
    assert [y[1] for y in got] == [payload]
    assert f.carried[1:3] == [200001, 400003] and f.carried[2] > 90 * T


# ---- 2. beyond one chunk of every scan and one pass of every grid ------------------------------------------------------------------------
def test_the_resolve_scan_beyond_its_first_chunk(rig):
    """k_hdlc_resolve's running map: the frame is the first gap of gap block 1,024, whose entry state is the whole first chunk.
    Through a run of flags sharing their zeros the machine cycles S, U3, U: one run length in three delivers the byte."""
    cfg = (1, 10, KEEP)
    body = np.array(hm.stuff(hm.bytes_to_bits(b"\x42")) + hm.FLAG, np.uint8)
    found = []
    for E in (SCAN * GAP_BLOCK, SCAN * GAP_BLOCK + 1, SCAN * GAP_BLOCK + 2):
        x = np.concatenate([np.tile(FLAG[:7], E), [0], body]).astype(np.uint8)
        ends = flag_ends(x)
        assert len(ends) == E + 1 > SCAN * GAP_BLOCK and E // GAP_BLOCK == SCAN          # the frame is gap E, in block 1,024
        assert (len(ends) + GAP_BLOCK - 1) // GAP_BLOCK > SCAN
        f = Feed(rig, cfg)
        found.append([y[1] for y in f.push(x)])
    assert sorted(found) == [[], [], [b"\x42"]], found


@pytest.mark.parametrize("split", ["whole", "at-the-seam"])
@pytest.mark.parametrize("cfg", [(0, 3, KEEP), (1, 10, FIX)], ids=lambda c: "%d-%d-%d" % c)
def test_the_offsets_scan_beyond_its_first_chunk(rig, T, drawn, cfg, split):
    """k_hdlc_offs's running count; 200,000 is no multiple of the tile, so the copies meet the seams at different phases"""
    x = np.resize(drawn, SCAN * T + 2 * T + 5)
    assert len(drawn) % T and (HALO + len(x) + T - 1) // T > SCAN + 2
    f = Feed(rig, cfg)
    if split == "whole":
        got = f.push(x)
    else:
        first = SCAN * T - HALO                            # with the 8 bits carried the first push fills one chunk exactly
        got = f.push(x[:first]) + f.push(x[first:])
        assert (f.carried[1] + len(x) - first + T - 1) // T >= 3
    assert len(got) > 10000 and sum(y[0] - rig.model[cfg].pos + len(x) + HALO > (SCAN + 1) * T for y in got) > 10     # frames that end behind the chunk


def test_every_grid_strides(rig, T, cus, drawn):
    """one push with more tiles than k_hdlc_mark and k_hdlc_ends have workgroups, more gap blocks than k_hdlc_gap has, and more
    flag ends than k_hdlc_emit has waves"""
    cfg = (1, 10, FIX)
    groups = GROUPS_PER_CU * cus
    E = GAP_BLOCK * groups + 1
    n = groups * T + 1
    x = np.concatenate([np.tile(FLAG[:7], E), [0], np.resize(drawn, n - 7 * E - 1)]).astype(np.uint8)
    ends = len(flag_ends(x))
    assert (HALO + len(x) + T - 1) // T > groups and (ends + GAP_BLOCK - 1) // GAP_BLOCK > groups and ends > 4 * groups
    assert len(Feed(rig, cfg).push(x)) > 1000


def test_the_record_list_is_full(rig, cus):
    """back-to-back flags with min_size 0 and the checksum kept: every flag end but the first delivers an empty frame"""
    cfg = (0, 3, KEEP)
    waves = 4 * GROUPS_PER_CU * cus
    n = 8 * (waves + 2)
    x = np.resize(FLAG, n)
    assert len(flag_ends(x)) == n // 8 > waves
    f = Feed(rig, cfg)
    got = f.push(x)
    assert len(got) == n // 8 - 1 and all(y[1] == b"" for y in got)
    # pushes whose first bit is a flag end: 8 k + 1 bits hold k + 1 frames, the bound of hdlc_host.hpp's hdlc_bounds exactly
    assert f.push(FLAG[:7]) == []
    for m in (1, 9, 17, 8 * (waves + 1) + 1):
        piece = np.resize(np.roll(FLAG, 1), m)
        assert list(flag_ends(np.concatenate([FLAG[:7], piece])) - 7) == list(range(0, m, 8))
        got = f.push(piece, "push" if m < 10 else "dev")
        assert len(got) == (m + 7) // 8
        assert len(rig.dev[cfg].frames()) == (m + 7) // 8
        assert f.push(FLAG[:7]) == []                      # up to the bit in front of the next flag end


@pytest.mark.parametrize("fill", [0x00, 0x55], ids=["zeros", "0x55"])
def test_frames_side_by_side_in_the_arena(rig, fill):
    """payloads that need no stuffing between single flags: a frame of k bytes has a gap of 8 k + 8 bits, fills its share
    (f - s - 8) / 8 of the arena to the last byte, and the next one starts one byte on"""
    cfg = (1, 10, KEEP)
    lens = list(range(1, 10))
    for phase in range(8):
        x = np.concatenate([np.ones(phase, np.uint8)] + [frame(bytes([fill] * k), with_crc=False)[:-8] for k in lens] + [FLAG])
        assert len(x) == phase + sum(8 * k + 8 for k in lens) + 8          # nothing was stuffed
        f = Feed(rig, cfg)
        got = f.push(x, "dev")
        assert [y[1] for y in got] == [bytes([fill] * k) for k in lens]
        rec, arena = rig.dev[cfg].frames(), rig.dev[cfg].frame_bytes()
        assert [int(r["len"]) for r in rec] == lens and int(rec[0]["start"]) == (HALO + phase + 8) // 8
        for a, b in zip(rec[:-1], rec[1:]):
            assert int(b["start"]) == int(a["start"]) + int(a["len"]) + 1
        # (the arena is sized by the host's bound of the carried bits, which is not the 8 that are carried)
        assert int(rec[-1]["start"]) + int(rec[-1]["len"]) <= (HALO + len(x)) // 8 <= len(arena) <= (rig.dev[cfg].dims()[1] + len(x)) // 8
        inside = np.zeros(len(arena), bool)
        for r in rec:
            inside[int(r["start"]):int(r["start"]) + int(r["len"])] = True
        assert np.all(arena[inside] == fill) and np.all(arena[~inside] == 0)


# ---- 3. the emitting wave's partitions -----------------------------------------------------------------------------------------------------
def _gap_words(x):
    """of a stream pushed whole behind clear(): (s + 1) mod 64 and the words of every gap between two flag ends"""
    e = flag_ends(x) + HALO
    s, f = e[:-1], e[1:]
    return (s + 1) & 63, ((f - 1) >> 6) - ((s + 1) >> 6) + 1


def _payload(kind, n, rng):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes() if kind == "random" else bytes([0x00 if kind == "zeros" else 0xff] * n)


def _seam_lengths(kind, rng):
    """the payload lengths around which a frame's gap goes from 64 to 65 and from 128 to 129 words (stuffing decides, so per kind)"""
    out = []
    for words in (64, 128):
        n = 64 * words * 5 // 48 - 8                       # (all ones stuff a sixth bit behind every five: no gap is longer)
        assert len(frame(_payload(kind, n, rng))) - 9 <= 64 * words
        while len(frame(_payload(kind, n, rng))) - 9 <= 64 * words:          # the gap: the stuffed body and 7 bits of the closing flag
            n += 1
        out.append(n)                                      # the first length that needs another word even when it starts a word
    return out


@pytest.fixture(scope="module")
def seam_lengths():
    rng = np.random.default_rng(44)
    return {kind: _seam_lengths(kind, rng) for kind in ("random", "zeros", "ones")}


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_intact_frames_of_every_lane_and_segment_partition(rig, seam_lengths, kind):
    """bytes per lane ceil(nbytes / 64) from 1 to 5, words per segment from 1 to 3, the two CRC bytes in one lane and in two,
    gaps starting at most bit phases of a word; one push per handle"""
    rng = np.random.default_rng(45)
    # a gap of a given length spans one word more when it starts late in a word: up to 8 bytes sooner
    lengths = list(range(261)) + [n + d for n in seam_lengths[kind] for d in range(-10, 3)]
    payloads = [_payload(kind, n, rng) for n in lengths]
    x = np.concatenate([np.concatenate([np.zeros(int(rng.integers(0, 71)), np.uint8), frame(p)]) for p in payloads])
    phase, words = _gap_words(x)
    assert {1, 2, 3} <= set(((words + 63) // 64).tolist()) and {64, 65, 128, 129} <= set(words.tolist())
    assert len(set(phase.tolist())) >= 48
    nbytes = np.array(lengths) + 2
    ch = (nbytes + 63) // 64
    assert set(ch.tolist()) >= {1, 2, 3, 4, 5}
    assert np.any((ch >= 2) & ((nbytes - 1) % ch == 0)) and np.any((ch >= 2) & ((nbytes - 1) % ch != 0))       # the CRC bytes in two lanes, in one
    for cfg in ((10, 1500, FIX), (0, 4096, 0), (0, 65535, KEEP)):
        got = Feed(rig, cfg).push(x)
        if cfg == (10, 1500, FIX):                         # (the idle zeros between two flags are frames of fewer than 10 bytes)
            assert [y[1] for y in got] == [p for p in payloads if len(p) + 2 >= 10]
        assert len(got) >= len([p for p in payloads if len(p) + 2 >= 10])


def _flip_places(n):
    """bits of a body of n bytes and its checksum: the first and last data bit, the two bits on either side of the first and of
    the last boundary between two lanes' bytes, four bits of the checksum"""
    nbytes = n + 2
    ch = (nbytes + 63) // 64
    last = (nbytes + ch - 1) // ch - 1                     # the last lane that has bytes
    places = {0, 8 * n - 1, 8 * n, 8 * n + 7, 8 * n + 8, 8 * n + 15}
    for i in {1, last} - {0}:
        places |= {8 * ch * i - 1, 8 * ch * i}
    return sorted(p for p in places if 0 <= p < 8 * nbytes)


def test_one_flipped_bit_at_the_lane_boundaries(rig, seam_lengths):
    rng = np.random.default_rng(46)
    lengths = [1, 2, 61, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 260] + [n + d for n in seam_lengths["random"] for d in (-1, 0)]
    pieces, data_flips, crc_flips, on_boundary = [], [], 0, 0
    for n in lengths:
        payload = _payload("random", n, rng)
        ch = (n + 2 + 63) // 64
        for h in _flip_places(n):
            pieces += [np.zeros(int(rng.integers(1, 8)), np.uint8), frame(payload, flip=h)]
            if h < 8 * n:
                data_flips.append(payload)
                on_boundary += ch >= 2 and h % (8 * ch) in (0, 8 * ch - 1) and h not in (0, 8 * n - 1)
            else:
                crc_flips += 1
    x = np.concatenate(pieces)
    assert on_boundary >= 4 * 10 and crc_flips >= 4 * len(lengths) and {2, 3} <= set(((_gap_words(x)[1] + 63) // 64).tolist())
    for cfg, want in (((0, 65535, FIX), (len(data_flips), crc_flips, len(data_flips) + crc_flips)), ((0, 4096, 0), (0, len(data_flips) + crc_flips, 0)),
                      ((10, 1500, FIX), None), ((0, 65535, KEEP), None)):
        f = Feed(rig, cfg)
        before = rig.dev[cfg].stats()
        got = f.push(x)
        if want is not None:
            assert delta(rig, cfg, before) == want
        if cfg == (0, 65535, FIX):                         # below the CRC's period one bit explains a wrong checksum: the payload comes back
            assert [(y[1], y[2]) for y in got] == [(p, True) for p in data_flips]


PERIOD = 32767          # of CRC-16/X.25's polynomial: data bits h and h + 32,767 change the checksum alike


@pytest.mark.parametrize("where,h", [("data", 100), ("data", 32766), ("data", 32767), ("data", 33599), ("crc", 0), ("crc", 7), ("crc", 8), ("crc", 15)])
def test_repairs_past_the_crc_period(rig, where, h):
    """the cross-lane minimum of k_hdlc_emit's hits against find_right_crc's loop order (hdlc_deframer.rs:41-71): the lowest of two
    data bits wins, and a data bit wins over the bit of the checksum that was really flipped, so a corrupt frame goes out"""
    cfg = (0, 65535, FIX)
    n = 4200
    payload = np.random.default_rng(47).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert 8 * n > PERIOD + 832                           # (bit 33,599 is the body's last)
    if where == "data":
        low = h - PERIOD if h >= PERIOD else h
        want = flipped(flipped(payload, h), low)            # (the payload itself where the flipped bit is the lowest)
        x = frame(payload, flip=h)
    else:
        want = flipped(payload, 833 + h)
        x = frame(payload, flip=8 * n + h)
    f = Feed(rig, cfg)
    before = rig.dev[cfg].stats()
    got = f.push(x)
    assert [(y[1], y[2]) for y in got] == [(want, True)]
    assert delta(rig, cfg, before) == (1, 0, 1)
    assert (want == payload) == (where == "data" and h < PERIOD)


# ---- 4. pushes that nobody fetched -----------------------------------------------------------------------------------------------------------
def test_three_pushes_and_one_fetch(rig, T, drawn):
    """the scratch grows with every push while the stream may still hold the one before; the results are the last push's, the
    counters everybody's"""
    cfg = (1, 10, FIX)
    rig.clear(cfg)
    d, m = rig.dev[cfg], rig.model[cfg]
    at, keep, want = 0, [], []
    windows = (500, 3 * T + 17, 20 * T)
    assert (windows[0] + T - 1) // T < (windows[1] + T - 1) // T < windows[2] // T          # more tiles every time: every buffer grows
    for n in windows:
        t, p = to_dev(np.ascontiguousarray(drawn[at:at + n]))
        keep.append(t)
        want = m.run(drawn[at:at + n])
        d.push_dev(p, n)
        at += n
    assert at < len(drawn) - 5000 and len(want) > 100
    assert d.result() == want
    assert d.stats() == m.stats()
    assert len(rig.feed(cfg, drawn[at:at + 5000])) > 10    # the carried state is whole
