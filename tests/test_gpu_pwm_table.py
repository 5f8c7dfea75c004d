"""GPU: the candidate table of k_pwm_walk (kernels_pwm.hip) past the boundaries tests/test_gpu_pwm.py stays below: more than 64 rows
(a second and third batch of the lanes' comparison), rows longer than 64 bytes whose length is no multiple of 8 (the lane-strided
copies, the pitch), open frames and tables of that size carried from one push to the next (fbits_in, meta_in, k_pwm_table), the
handle's limits filled to the end of the walk's LDS, hundreds of deliveries into one arena, and the fuzz family over several tiles
in both element sizes.

Every stream comes from tests/pwm_streams.py, and tests/test_pwm_table_cpu.py asserts on the model alone what each of them holds,
so no comparison here is against an empty expectation.  A Pair compares every push exactly: the bits, `repeats`, `first_sample`
and the order of the frames, and the push that delivers them.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest

import pwm_model as pm
import pwm_streams as ps
from pwm_streams import Pair

pytestmark = pytest.mark.gpu


def flat(parts):
    return [f for part in parts for f in part]


@pytest.fixture(scope="module")
def T():
    t = Pair(*ps.BASE).dev.dims()
    assert t == ps.TILE                        # the cut points of pwm_streams.py are the kernels' tile seams
    return t


# ---- 1. the table past one wave ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wave():
    c = ps.table_past_one_wave()
    return c, pm.PwmModel(*c.pos, **c.kw).push(c.x)


def check_arena(dev, want):
    """frames()["start"] is the running sum of "len", frame_bits() the frames one behind the other, bits_dev() as long"""
    rec, arena = dev.frames(), dev.frame_bits()
    lens = [len(f[0]) for f in want]
    assert rec["len"].tolist() == lens and rec["start"].tolist() == np.cumsum([0] + lens)[:-1].tolist()
    assert rec["repeats"].tolist() == [f[1] for f in want] and rec["first_sample"].tolist() == [f[2] for f in want]
    assert arena.tolist() == [b for f in want for b in f[0]]
    ptr, nbits = dev.bits_dev()
    assert nbits == sum(lens) and (ptr is not None) == (nbits > 0)


def test_165_words_in_one_launch_match_rows_of_every_batch(wave):
    """(a) rows 3 | 63, 64, 70 | 127, 128, 159 repeat: the repeats find rows the same launch wrote, in the first, second and third
    batch of 64 candidates; word 160 found no row and finds none"""
    c, want = wave
    p = Pair(c.pos, c.kw)
    assert p.feed(c.x, "dev") == want and len(want) == 160
    check_arena(p.dev, want)
    assert p.dev.bits_dev()[1] == 160 * 70
    assert p.model.counters["distinct_cap"] == 6
    assert p.flush() == []


@pytest.mark.parametrize("cuts", [["carry", "table", "repeats"], ["carry"], ["table"]], ids=lambda c: "+".join(c))
def test_165_words_cut_in_an_open_frame_of_66_bits_and_behind_the_table(wave, cuts):
    """(b) the open frame carries more than 64 bits over a push (fbits_in), every repeat matches a row that came through
    k_pwm_table, and the repeats themselves are cut in two"""
    c, want = wave
    p = Pair(c.pos, c.kw)
    parts = p.feed_cut(c.x, [c.cuts[k] for k in cuts], "dev")
    assert [len(q) for q in parts] == [0] * len(cuts) + [160] and parts[-1] == want
    check_arena(p.dev, want)


def test_165_words_over_nine_pushes_change_halves_with_more_than_64_rows(wave):
    """(c) eight changes of the table's half, each with 67 to 160 rows in it, by host pushes"""
    c, want = wave
    p = Pair(c.pos, c.kw)
    parts = p.feed_cut(c.x, c.cuts["halves"])
    assert len(parts) == 9 and flat(parts[:-1]) == [] and parts[-1] == want


def test_165_words_with_min_repeats_2_deliver_the_seven_repeated_rows(wave):
    """(d) deliver() skips rows and still reads the right ones"""
    c, want = wave
    d = ps.table_past_one_wave(min_repeats=2)
    for cuts in ([], [d.cuts["table"]]):
        p = Pair(d.pos, d.kw)
        out = flat(p.feed_cut(d.x, cuts, "dev"))
        assert out == [want[i] for i in ps.WAVE_ROWS] and [f[1] for f in out] == ps.WAVE_REPEATS
        check_arena(p.dev, out)


def test_165_words_without_a_reset_come_out_of_the_flush(wave):
    """(e) the last gap is the frame gap: no push delivers, the flush walks a table that k_pwm_table carried whole"""
    c, want = wave
    e = ps.table_past_one_wave(last_gap=ps.FGAP)
    for cuts in ([], [e.cuts["carry"], e.cuts["table"]]):
        p = Pair(e.pos, e.kw)
        assert flat(p.feed_cut(e.x, cuts, "dev")) == []
        assert p.dev.bits_dev() == (None, 0) and len(p.dev.frames()) == 0
        assert p.flush() == want
        check_arena(p.dev, want)


# ---- 2. mixed lengths, prefixes, single-bit differences --------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut between the passes"])
def test_prefixes_and_single_bit_differences_find_their_own_rows(cut):
    """Words of 1 .. 200 bits of which every shorter one is a prefix of every longer one, and four words that differ from the
    129-bit one in bit 0, 63, 64 or 128 alone (the first and last byte of a row's first and third stride of 64): each counts
    its own repeat and no other row's.  The pre-filter on length and hash stands in front of the comparison of the bits and
    cannot be taken out of the way on purpose: a collision of the 64-bit pwm_hash_step chain cannot be constructed, so a wrong
    comparison of the bits shows here only through the rows it fails to match, not through rows it matches wrongly."""
    c = ps.prefixes_and_flips()
    p = Pair(c.pos, c.kw)
    parts = p.feed_cut(c.x, [c.cuts["passes"]] if cut else [], "dev")
    out = flat(parts)
    assert [(f[0], f[1]) for f in out] == [(w, 2) for w in c.words[:13]] and parts[:-1] == [[]] * cut
    check_arena(p.dev, out)


# ---- 3. the handle's limits, filled -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut behind bit 16000"])
def test_a_frame_of_16384_bits_repeats_and_one_more_bit_overflows(cut):
    """max_frame_bits at its limit: the open frame fills the walk's s_bits to its end, the 16,385th bit invalidates the second
    word, the third finds the row of the first"""
    c = ps.longest_frame()
    p = Pair(c.pos, c.kw)
    parts = p.feed_cut(c.x, [c.cuts["carry"]] if cut else [], "dev")
    assert flat(parts) == [(c.words[0], 2, 0)] and p.model.counters["overflow"] == 1
    check_arena(p.dev, parts[-1])


@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut behind word 1030"])
def test_a_table_of_1024_rows_fills_and_its_first_and_last_rows_repeat(cut):
    """max_distinct_frames at its limit: s_cand is used to its end, six words are turned away, rows 0, 63, 64 and 1023 repeat and
    word 1024, which was turned away, is turned away again"""
    c = ps.fullest_table()
    p = Pair(c.pos, c.kw)
    parts = p.feed_cut(c.x, [c.cuts["table"]] if cut else [], "dev")
    out = flat(parts)
    assert len(out) == 1024 and [i for i, f in enumerate(out) if f[1] == 2] == [0, 63, 64, 1023]
    assert p.model.counters["distinct_cap"] == 7 and parts[:-1] == [[]] * cut
    check_arena(p.dev, out)


# ---- 4. many deliveries in one push -----------------------------------------------------------------------------------------------------
def test_200_transmissions_in_one_push_and_over_random_cuts():
    """deliver() runs 200 times in one launch: the records and the arena offsets go on from one delivery to the next"""
    c = ps.many_transmissions()
    p = Pair(c.pos, c.kw)
    want = p.feed(c.x, "dev")
    assert len(want) > 3 * 64
    check_arena(p.dev, want)
    q = Pair(c.pos, c.kw)
    at, got = 0, []
    for k, cut in enumerate(c.cuts["random"] + [len(c.x)]):
        part = q.feed(c.x[at:cut], "dev" if k % 2 else "push")        # (the push a frame arrives in is the model's, in feed)
        check_arena(q.dev, part)                                       # every push's arena starts at 0
        got += part
        at = cut
    assert got == want and q.model.reset_samples == p.model.reset_samples


# ---- 5. the fuzz family across tiles, both element sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(pm.FUZZ_SEEDS))
def test_fuzz_over_three_tiles_whole_cut_at_the_seams_and_in_random_pushes(seed, T):
    c = ps.fuzz_tiled(seed, T)
    whole = Pair(c.pos, c.kw)
    one = whole.feed(c.x, "dev") + whole.flush()
    for cut in c.cuts["seams"]:
        p = Pair(c.pos, c.kw)
        assert flat(p.feed_cut(c.x, [cut], "dev")) + p.flush() == one, cut
    p = Pair(c.pos, c.kw)
    assert flat(p.feed_cut(c.x, c.cuts["random"])) + p.flush() == one


@pytest.mark.parametrize("seed", list(pm.FUZZ_SEEDS))
def test_fuzz_over_three_tiles_as_complex_samples(seed, T):
    """the Complex loader on jittered content with NaN and Inf over several tiles: the expectation is the model on numpy's f32
    zr * zr + zi * zi"""
    c = ps.fuzz_tiled(seed, T)
    z, power = ps.complex_of(c.x)
    whole = Pair(c.pos, c.kw, np.complex64)
    one = whole.feed(power, "dev", z) + whole.flush()
    for cut in (T, T + 1):
        p = Pair(c.pos, c.kw, np.complex64)
        assert flat(p.feed_cut(power, [cut], "push" if cut == T else "dev", z)) + p.flush() == one, cut
