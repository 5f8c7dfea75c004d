"""No GPU: every stream generator of tests/pwm_streams.py through pwm_model.PwmModel alone.  tests/test_gpu_pwm_table.py compares the
device with the model on these streams; what is asserted here is that the model's side of those comparisons is not empty: the
frames, the rows that repeat, the counters and the carried state each stream was built to reach."""
import os
import re

import numpy as np

import pwm_model as pm
import pwm_streams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_of(case):
    return pm.PwmModel(*case.pos, **case.kw)


def test_tile_is_the_kernels_tile():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "pwm_core.hpp")).read()
    b, per = (int(re.search(r"\b%s = (\d+)" % k, src).group(1)) for k in ("PWM_B", "PWM_PER"))
    assert b * per == ps.TILE


def test_the_table_past_one_wave():
    c = ps.table_past_one_wave()
    assert len(c.x) == 86837 and len(c.x) / ps.TILE > 42.4 and len(set(c.words[:165])) == 165
    m = model_of(c)
    out = m.push(c.x)
    assert len(out) == 160 and [f[0] for f in out] == c.words[:160] and m.flush() == []
    rows = [i for i, f in enumerate(out) if f[1] > 1]
    assert rows == ps.WAVE_ROWS and [out[i][1] for i in rows] == ps.WAVE_REPEATS
    assert m.counters["distinct_cap"] == 6 and m.counters["overflow"] == 0 and m.counters["invalid_width"] == 0
    assert [f[2] for f in out] == [i * (70 * ps.BIT + ps.FGAP) for i in range(160)]
    # (d) min_repeats 2: those seven rows, in table order
    d = ps.table_past_one_wave(min_repeats=2)
    md = model_of(d)
    assert md.push(d.x) == [out[i] for i in rows] and md.counters["below_min_repeats"] == 153
    # (e) no reset: nothing comes before the flush
    e = ps.table_past_one_wave(last_gap=ps.FGAP)
    me = model_of(e)
    assert len(e.x) == len(c.x) - (ps.RGAP - ps.FGAP) and me.push(e.x) == [] and me.flush() == out
    # (b) the cuts: an open frame of more than 64 bits, a table of 160 rows in front of the repeats, a cut between them
    m = model_of(c)
    assert m.push(c.x[:c.cuts["carry"]]) == [] and 64 < len(m.bits) < 70 and len(m.candidates) == 100
    m = model_of(c)
    assert m.push(c.x[:c.cuts["table"]]) == [] and len(m.candidates) == 160 and all(k[1] == 1 for k in m.candidates)
    assert c.cuts["carry"] < c.cuts["table"] < c.cuts["repeats"] < len(c.x)
    m = model_of(c)
    m.push(c.x[:c.cuts["repeats"]])
    assert [i for i, k in enumerate(m.candidates) if k[1] > 1] == [3, 63, 64, 70]
    # (c) every cut finds more than 64 rows, so every change of halves copies rows of a second batch
    assert len(c.cuts["halves"]) >= 5 and c.cuts["halves"] == sorted(set(c.cuts["halves"]))
    m, at = model_of(c), 0
    for cut in c.cuts["halves"]:
        assert m.push(c.x[at:cut]) == [] and len(m.candidates) > 64
        at = cut


def test_mixed_lengths_prefixes_and_single_bit_differences():
    c = ps.prefixes_and_flips()
    once = c.words[:13]
    assert len(set(once)) == 13 and c.words[13:] == once[::-1]
    assert [len(w) for w in once] == ps.PREFIX_LENGTHS + [129] * 4
    assert all(once[j][:len(once[i])] == once[i] for i in range(9) for j in range(i, 9))          # every shorter word is a prefix
    assert [[k for k in range(129) if w[k] != once[7][k]] for w in once[9:]] == [[k] for k in ps.FLIPPED]
    m = model_of(c)
    out = m.push(c.x)
    assert [(f[0], f[1]) for f in out] == [(w, 2) for w in once] and not any(m.counters.values())
    m = model_of(c)
    assert m.push(c.x[:c.cuts["passes"]]) == [] and [k[1] for k in m.candidates] == [1] * 13 and not m.bits


def test_the_limits_filled():
    c = ps.longest_frame()
    assert len(c.x) == 344109
    m = model_of(c)
    assert m.push(c.x) == [(c.words[0], 2, 0)] and m.counters["overflow"] == 1 and sum(m.counters.values()) == 1
    m = model_of(c)
    assert m.push(c.x[:c.cuts["carry"]]) == [] and 15999 <= len(m.bits) <= 16000
    c = ps.fullest_table()
    assert len(c.x) == 96266 and len(set(c.words[:1030])) == 1030
    m = model_of(c)
    out = m.push(c.x)
    assert len(out) == 1024 and [f[0] for f in out] == c.words[:1024]
    assert [i for i, f in enumerate(out) if f[1] > 1] == [0, 63, 64, 1023] and {f[1] for f in out} == {1, 2}
    assert m.counters["distinct_cap"] == 7
    m = model_of(c)
    assert m.push(c.x[:c.cuts["table"]]) == [] and len(m.candidates) == 1024 and m.counters["distinct_cap"] == 6


def test_many_deliveries_in_one_push():
    c = ps.many_transmissions()
    assert len(c.words) == 200 and all(1 <= len(set(tx)) <= 3 and all(3 <= len(w) <= 9 for w in tx) for tx in c.words)
    m = model_of(c)
    out = m.push(c.x)
    assert len(m.reset_samples) == 200 and len(out) == sum(len(set(tx)) for tx in c.words) > 3 * 64
    assert {f[1] for f in out} == {1, 2, 3} and not any(m.counters.values())
    assert len({len(f[0]) for f in out}) == 7                            # the arena offsets grow by every length from 3 to 9
    # over the cuts the deliveries spread: many pushes deliver several transmissions, some none
    m, at, per_push = model_of(c), 0, []
    for cut in c.cuts["random"] + [len(c.x)]:
        per_push.append(len(m.push(c.x[at:cut])))
        at = cut
    assert sum(per_push) == len(out) and len(per_push) > 10 and max(per_push) > 10 and min(per_push) == 0


def test_the_fuzz_family_across_tiles_delivers_in_both_element_sizes():
    delivering, frames, with_nan = [0, 0], [0, 0], 0
    for seed in pm.FUZZ_SEEDS:
        c = ps.fuzz_tiled(seed)
        assert len(c.x) >= 3 * ps.TILE + 17 and len(c.x) % len(pm.fuzz_case(seed)[2]) == 0
        assert all(0 < cut < len(c.x) for cut in c.cuts["seams"] + c.cuts["random"])
        z, power = ps.complex_of(c.x)
        assert z.dtype == np.complex64 and power.dtype == np.float32
        assert np.array_equal(np.isnan(power), np.isnan(c.x)) and np.array_equal(power == np.inf, c.x == np.inf)
        assert not power[c.x == -np.inf].any()
        with_nan += bool(np.isnan(c.x).any())
        for k, x in enumerate((c.x, power)):
            m = model_of(c)
            out = m.push(x) + m.flush()
            delivering[k] += bool(out)
            frames[k] += len(out)
    print("f32: %d seeds, %d frames; Complex: %d seeds, %d frames; NaN in %d seeds" % (delivering[0], frames[0], delivering[1], frames[1], with_nan))
    assert min(delivering) >= 12 and min(frames) >= 300, (delivering, frames)
    assert 2 * with_nan >= len(pm.FUZZ_SEEDS), with_nan
