"""GPU: rr_pwm_decoder (kernels_pwm.hip) against the sequential model of tests/pwm_model.py.  Every comparison is exact: the bits,
`repeats`, `first_sample` and the order of the frames, and the push that delivers them; there is no tolerance anywhere in this file.

A Pair (tests/pwm_streams.py) is a handle and a PwmModel fed the same samples, so the expectation follows the handle whatever came before: a stream that
ends in reset_gap of silence leaves both with no pulse, no frame and no candidate, and the next stream starts clean."""
import numpy as np
import pytest
import torch

import pwm_model as pm
import rustradio_amd as rr
from pwm_streams import BASE, FGAP, LONG, RGAP, SHORT, Pair, frames_of, runs, word

pytestmark = pytest.mark.gpu
DOC = pm.load_known_answers()


def launches():
    return rr.lib().rr_debug_kernel_launches()


@pytest.fixture(scope="module")
def base():
    return Pair(*BASE)


@pytest.fixture(scope="module")
def T(base):
    t = base.dev.dims()
    assert t % 64 == 0 and t >= 256
    return t


# ---- 1. the reference's own tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DOC["cases"], ids=[c["name"] for c in DOC["cases"]])
def test_golden_cases(case):
    pos, kw = pm.golden_settings(DOC, case["settings"])
    p = Pair(pos, kw)
    out = p.feed(pm.golden_samples(DOC, case)) + p.flush()
    if "expect" in case:
        assert ["".join(map(str, b)) for b, _, _ in out] == [e["bits"] for e in case["expect"]]
        assert all(e["repeats"] is None or e["repeats"] == f[1] for f, e in zip(out, case["expect"]))
    else:
        assert len(out) == case["expect_count"] and "".join(map(str, out[0][0])) == case["first_bits"]


def test_validate_refusals_come_before_the_device_in_the_references_words():
    before = launches()
    for v in DOC["validate"]:
        pos, kw = pm.golden_settings(DOC, v["settings"])
        if v["ok"]:
            assert rr.PwmDecoder(*pos, **kw).name == "PwmDecoder"
        else:
            with pytest.raises(ValueError) as e:
                rr.PwmDecoder(*pos, **kw)
            assert str(e.value) == pm.MESSAGES[v["error"]]
    assert launches() == before
    for kw in (dict(max_frame_bits=4096, max_distinct_frames=256), dict(max_frame_bits=16384), dict(max_distinct_frames=1024)):
        assert rr.PwmDecoder(0.5, 2, 5, 9, 20, **kw).dims() > 0          # the defaults and the limits themselves are accepted


# ---- 2. the fuzz family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(pm.FUZZ_SEEDS))
def test_fuzz_in_one_push_and_in_random_splits(seed):
    pos, kw, x = pm.fuzz_case(seed)
    whole = Pair(pos, kw)
    one = whole.feed(x, "dev" if seed % 2 else "push") + whole.flush()
    rng = np.random.default_rng(seed)
    cuts, at = [], 0
    while at < len(x):
        at += 1 if rng.random() < 0.3 else int(rng.integers(1, 200))      # pushes of one sample included
        if at < len(x):
            cuts.append(at)
    split = Pair(pos, kw)
    parts = split.feed_cut(x, cuts)
    assert [f for part in parts for f in part] + split.flush() == one


# ---- 3. every 2-way cut ---------------------------------------------------------------------------------------------------------------
def test_every_two_way_cut_of_a_stream_with_two_transmissions(base):
    a, b = [1, 0, 1, 1], [0, 1, 1]
    x = runs(*word(a), *word(a), *word(b, RGAP), *word(b), *word(a, FGAP + 3), *word(b, RGAP))
    assert 200 < len(x) < 400
    ref = pm.PwmModel(*base.pos, **base.kw)
    whole = ref.push(x)
    assert [(f[0], f[1]) for f in whole] == [(tuple(a), 2), (tuple(b), 1), (tuple(b), 2), (tuple(a), 1)] and len(ref.reset_samples) == 2
    for cut in range(len(x) + 1):
        off = base.model.sample_index
        first, second = base.feed_cut(x, [cut])
        # a push delivers the transmissions whose reset sample lies inside it
        n1 = sum(1 for r in ref.reset_samples if r < cut)
        assert len(first) == 2 * n1 and len(second) == 4 - 2 * n1, cut
        assert [(f[0], f[1], f[2] - off) for f in first + second] == whole, cut


# ---- 4. seams ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feature", ["rise", "fall", "frame_gap_sample", "reset_sample"])
def test_features_on_the_tile_seams(base, T, feature):
    tx = word([1, 0, 1]) + word([1, 0, 1], RGAP)
    lens = np.cumsum([0] + [c for _, c in tx])
    at = {"rise": lens[2], "fall": lens[3], "frame_gap_sample": lens[5] + FGAP - 1, "reset_sample": lens[-3] + RGAP - 1}[feature]
    for where in (T - 1, T, T + 1):
        x = np.concatenate([np.zeros(where - at, np.float32), runs(*tx), np.zeros(3, np.float32)])
        out = base.feed(x, "dev")                                  # the feature on tile 0's last, tile 1's first and second sample
        assert [(f[0], f[1]) for f in out] == [((1, 0, 1), 2)]
        for cut in (where - 1, where, where + 1, T):               # ... and the push seam there as well, and on the tile seam
            parts = base.feed_cut(x, [cut])
            assert [(f[0], f[1]) for p in parts for f in p] == [((1, 0, 1), 2)]


def test_pulse_and_gaps_straddling_a_tile_seam_and_a_push_seam(base, T):
    for what, lead in (("pulse", T - 2), ("frame gap", T - 12), ("reset gap", T - 37)):
        # lead low samples, then 0 1 | gap | 0 1 | reset: the straddling run begins a few samples in front of sample T
        x = np.concatenate([np.zeros(lead, np.float32), runs(*word([0, 1]), *word([0, 1], RGAP + 5))])
        assert len(x) > T + 4
        assert [(f[0], f[1]) for f in base.feed(x)] == [((0, 1), 2)], what
        parts = base.feed_cut(x, [T])
        assert [(f[0], f[1]) for p in parts for f in p] == [((0, 1), 2)], what
        parts = base.feed_cut(x, [T - 1, T, T + 1])
        assert [(f[0], f[1]) for p in parts for f in p] == [((0, 1), 2)], what


def test_runs_longer_than_one_chunk_of_the_tile_scan(T):
    """a high run and a low run of more than 1024 tiles each: the fall and the reset sample land in the scan's last chunk"""
    chunk = 1024 * T
    rgap = chunk + 3 * T + 17
    p = Pair([0.5, SHORT, LONG, FGAP, rgap], dict(low_threshold=0.25, pulse_tolerance=1, max_frame_bits=16, max_distinct_frames=4))
    x = runs(*word([1, 1, 0]), *word([1, 1, 0]), (True, chunk + 5 * T + 3), (False, FGAP), *word([0, 1]), (False, rgap + 2))
    out = p.feed(x, "dev")
    assert [(f[0], f[1]) for f in out] == [((1, 1, 0), 2), ((0, 1), 1)]
    assert p.model.counters["invalid_width"] == 1 and len(p.model.reset_samples) == 1
    assert p.model.reset_samples[0] // T > 2 * 1024                    # in the third chunk of this push's scan
    out = p.feed_cut(np.concatenate([runs(*word([1, 0])), np.zeros(rgap, np.float32)]), [7, 7 + chunk + 1])
    assert [len(o) for o in out] == [0, 0, 1]                          # the low run carried over two pushes as a 64-bit count


# ---- 5. carried state -----------------------------------------------------------------------------------------------------------------
def test_a_transmission_spread_over_three_pushes(base):
    w = runs(*word([1, 1, 0, 1]))
    x = np.concatenate([w, w, w, w, np.zeros(RGAP, np.float32)])
    out = base.feed_cut(x, [len(w) + 3, 3 * len(w) - 2])
    assert [len(o) for o in out] == [0, 0, 1] and out[2][0][:2] == ((1, 1, 0, 1), 4)


def test_frames_of_max_frame_bits_and_one_more_over_two_pushes(base):
    for nbits, want in ((16, 1), (17, 0)):
        bits = [1, 0] * 8 + [1] * (nbits - 16)
        x = runs(*word(bits, RGAP))
        for cut in (3, len(x) // 2, len(x) - RGAP - 1):
            out = base.feed_cut(x, [cut])
            assert len(out[0]) == 0 and len(out[1]) == want, (nbits, cut)
            if want:
                assert out[1][0][0] == tuple(bits)
    assert base.model.counters["overflow"] >= 3


def test_the_candidate_cap_in_one_push_and_repeats_in_the_next(base):
    words = [[1, 1, 1], [0, 0, 0], [1, 0, 1], [0, 1, 0], [1, 1, 0]]       # max_distinct_frames is 4: the fifth is turned away
    first = runs(*[r for w in words for r in word(w)])
    second = runs(*word(words[1]), *word(words[4]), *word(words[4], RGAP))
    cap0 = base.model.counters["distinct_cap"]
    out = base.feed_cut(np.concatenate([first, second]), [len(first)])
    assert out[0] == [] and [(f[0], f[1]) for f in out[1]] == [((1, 1, 1), 1), ((0, 0, 0), 2), ((1, 0, 1), 1), ((0, 1, 0), 1)]
    assert base.model.counters["distinct_cap"] - cap0 == 3


def test_flush_delivers_without_a_reset_drops_the_open_frame_and_ends_the_handle():
    p = Pair(*BASE)
    x = runs(*word([1, 0, 0]), *word([1, 0, 0]), (True, SHORT), (False, LONG), (True, SHORT))
    assert p.feed(x) == []
    out = p.flush()
    assert [(f[0], f[1], f[2]) for f in out] == [((1, 0, 0), 2, 0)]
    rec, arena = p.dev.frames(), p.dev.frame_bits()
    assert len(rec) == 1 and arena.tolist() == [1, 0, 0] and p.dev.bits_dev()[1] == 3
    before = launches()
    for call in (lambda: p.dev.push(np.zeros(4, np.float32)), lambda: p.dev.push(np.zeros(0, np.float32)), p.dev.flush):
        with pytest.raises(ValueError, match="push after flush"):
            call()
    assert launches() == before
    with pytest.raises(RuntimeError, match="PwmDecoder delivers frames"):
        p.dev.work(np.zeros(4, np.float32), 4)


def test_refused_and_empty_pushes_touch_nothing(base):
    L = rr.lib()
    half = runs(*word([1, 1]))
    assert base.feed(half) == []
    before = launches()
    assert L.rr_pwm_decoder_push_dev(base.dev._h, None, 5, None) != 0 and "null samples" in rr.last_error()
    assert L.rr_pwm_decoder_push_dev(base.dev._h, None, (1 << 30) + 1, None) != 0 and "2^30" in rr.last_error()
    assert base.feed(np.zeros(0, np.float32)) == [] and base.feed(np.zeros(0, np.float32), "dev") == []
    assert launches() == before and base.dev.bits_dev() == (None, 0)
    out = base.feed(np.concatenate([half, np.zeros(RGAP, np.float32)]))
    assert [(f[0], f[1]) for f in out] == [((1, 1), 2)]


# ---- 6. density -----------------------------------------------------------------------------------------------------------------------
def test_launch_count_is_seven_whatever_the_samples_hold(T):
    n = 3 * T + 17
    alt = np.resize(np.array([1.0, 0.0], np.float32), n)
    nan = np.resize(np.array([np.nan, 0.3], np.float32), n)          # a NaN swaps the slicer, the band keeps it: an edge on every second
    nan2 = np.full(n, np.nan, np.float32)                             # ... and on every sample
    burst = np.concatenate([runs(*word([1, 0, 1]), *word([1, 0, 1], RGAP)), np.zeros(n, np.float32)])[:n]
    counts = []
    p = Pair([0.5, 1, 2, 3, 6], dict(low_threshold=0.25, pulse_tolerance=0, max_frame_bits=8, max_distinct_frames=2))
    for x in (np.zeros(n, np.float32), burst, alt, nan, nan2, np.concatenate([alt[:T + 5], np.zeros(40, np.float32), alt[:n - T - 45]])):
        t = torch.from_numpy(x).cuda()
        want = p.model.push(x)
        before = launches()
        p.dev.push_dev(t.data_ptr(), n)
        counts.append(launches() - before)
        assert frames_of(p.dev.result()) == want
        p.feed(np.zeros(8, np.float32))
    assert counts == [7] * 6, counts
    assert p.model.counters["overflow"] > 0 and p.model.counters["invalid_width"] > 0


# ---- 7. Complex input ------------------------------------------------------------------------------------------------------------------
def test_complex_input_equals_mag2_in_front_of_the_power_handle():
    """the power of the Complex samples crosses both thresholds within one f32 ulp: both element sizes must see the same bits"""
    pos, kw = [0.5, SHORT, LONG, FGAP, RGAP], dict(low_threshold=0.25, pulse_tolerance=1, max_frame_bits=16, max_distinct_frames=4)
    rng = np.random.default_rng(7)
    head = runs(*word([1, 0, 1, 1]), *word([1, 0, 1, 1]), *word([0, 1], RGAP), *word([0, 1, 1]), *word([0, 1, 1], RGAP))
    env = np.concatenate([head, runs(*word([1, 1, 0]), *word([1, 1, 0], RGAP + 1))])      # the last transmission stays clean
    # in a pulse the slicer asks about the low threshold, in a gap about the high one: one ulp below, on, and one ulp above it
    thr = np.where(env > 0, np.float32(0.25), np.float32(0.5)).astype(np.float32)
    steps = rng.integers(-1, 2, len(env))
    target = np.where(steps < 0, np.nextafter(thr, np.float32(0)), np.where(steps > 0, np.nextafter(thr, np.float32(1)), thr))
    touched = (rng.random(len(env)) < 0.15) & (np.arange(len(env)) < len(head))
    target = np.where(touched, target, env).astype(np.float32)
    # amplitude times 1, i, -1 or -i: the power is ONE rounded square, within an ulp of the target
    amp = np.sqrt(target.astype(np.float64)).astype(np.float32)
    z = (amp.astype(np.complex64) * np.array([1, 1j, -1, -1j], np.complex64)[rng.integers(0, 4, len(env))]).astype(np.complex64)
    mag = rr.ComplexToMag2()
    power = mag.work(z, len(z))[4]
    assert len(power) == len(z)
    near = touched & (np.abs(power.astype(np.float64) - thr) <= 2 * np.spacing(thr))
    assert near.sum() > touched.sum() // 2 > 10 and (power[near] > thr[near]).any() and (power[near] < thr[near]).any() and (power[near] == thr[near]).any()
    f32, c64 = Pair(pos, kw), rr.PwmDecoder(*pos, **kw, dtype=np.complex64)
    want = f32.feed(power) + f32.flush()
    got = frames_of(c64.push(z)) + frames_of(c64.flush())
    assert got == want and len(want) >= 1 and c64.name == "ComplexToMag2>PwmDecoder"
    halves = rr.PwmDecoder(*pos, **kw, dtype=np.complex64)
    cut = len(z) // 2 + 1
    assert frames_of(halves.push(z[:cut])) + frames_of(halves.push(z[cut:])) + frames_of(halves.flush()) == want


# ---- 8. examples/restaurant_pager.rs -----------------------------------------------------------------------------------------------
def test_restaurant_pager_settings_on_one_transmission_in_noise():
    """125 kS/s: short 26, long 80, frame gap 110, reset gap 914, 25 bits, min_repeats 3, Delimiter; five repeats of one word"""
    rng = np.random.default_rng(3)
    bits = [int(b) for b in rng.integers(0, 2, 25)]
    lead = 5000
    r = [(False, lead)]
    for _ in range(5):
        for b in bits:
            r += [(True, 26 if b else 80), (False, 80 if b else 26)]
        r += [(True, 26), (False, 300)]
    r.append((False, 1500))
    env = runs(*r)
    noise = (rng.normal(0, 0.05, len(env)) + 1j * rng.normal(0, 0.05, len(env)))
    z = (env * 1.0 + noise).astype(np.complex64)                     # power about 1 in a pulse, about 0.005 in a gap
    d = rr.PwmDecoder(0.5, 26, 80, 110, 914, frame_bits=25, min_repeats=3, delimiter=True, dtype=np.complex64)
    out = frames_of(d.push(z))
    assert out == [(tuple(bits), 5, lead)]
    m = pm.PwmModel(0.5, 26, 80, 110, 914, frame_bits=25, min_repeats=3, delimiter=True)
    zr, zi = z.real.astype(np.float32), z.imag.astype(np.float32)
    assert m.push((zr * zr + zi * zi).astype(np.float32)) == out
