"""CPU-only: the test-side model of Wpcr (tests/wpcr_model.py) against itself — the drift-free clock of rr_wpcr against the
reference's f32 accumulator, find_best_bin's edge cases, the margins of the burst builder the GPU tests rely on — and the
no-fallback rule for rr.Wpcr."""
import numpy as np
import pytest

import rustradio_amd as rr
import wpcr_model as wm

F32 = np.float32
U = 2.0 ** -24


def test_exact_picks_differ_from_the_f32_accumulator_only_next_to_an_integer_phase():
    """300 random (n <= 20000, bin, p0): every sample in the symmetric difference of the two pick sets has P(i) or P(i - 1)
    within (i + 1) 2^-24 of an integer, and the end phases differ by at most n 2^-24"""
    rng = np.random.default_rng(7)
    differing = 0
    for _ in range(300):
        n = int(rng.integers(4, 20001))
        b = int(rng.integers(2, max(3, (n - 1) // 2 - 1)))
        f = F32(b) / F32(n)
        t = F32(rng.uniform(0.0, 1.0))
        p0 = t if t > F32(0.5) else F32(t + F32(1.0))
        x = np.zeros(n, F32)
        seq, end_seq = wm.accumulate_f32(x, p0, f)
        exact, nsyms, end_exact = wm.picks_exact(p0, f, n)
        assert nsyms == len(exact)
        diff = np.setxor1d(seq, exact)
        differing += len(diff) > 0
        if len(diff):
            near = np.minimum(wm.near_integer(p0, f, diff), wm.near_integer(p0, f, diff - 1))
            assert np.all(near <= (diff + 1) * U), (n, b, float(p0), diff[:5], near[:5])
        # (a last pick that one side makes at sample n - 1 and the other would make at sample n leaves the counts one apart and
        #  the phases 1 apart: the same clock)
        d = abs(float(end_seq) - float(end_exact))
        if len(seq) != nsyms:
            assert abs(len(seq) - nsyms) == 1
            d = abs(d - 1.0)
        assert d <= n * U, (n, b, float(p0), float(end_seq), float(end_exact))
    print(f"{differing} of 300 differ")


def test_picks_exact_against_a_plain_fraction_loop():
    from fractions import Fraction
    for p0, f, n in ((F32(1.0), F32(0.25), 9), (F32(0.75), F32(3) / F32(17), 40), (F32(1.5), F32(2) / F32(4), 4),
                     (F32(0.50000006), F32(2) / F32(511999), 600)):
        P, prev, want = Fraction(float(p0)), 0, []
        for i in range(n):
            fl = (Fraction(float(p0)) + i * Fraction(float(f))).__floor__()
            if fl > prev:
                want.append(i)
            prev = fl
        taken, nsyms, end = wm.picks_exact(p0, f, n)
        assert taken.tolist() == want and nsyms == prev
        assert end == wm.fl32(P + n * Fraction(float(f)) - nsyms)


def test_fl32_rounds_to_nearest_even():
    from fractions import Fraction
    assert wm.fl32(Fraction(1, 3)) == F32(1.0) / F32(3.0)
    assert wm.fl32(Fraction(2 ** 24 + 1, 2 ** 24)) == F32(1.0)                  # a tie: to even
    assert wm.fl32(Fraction(2 ** 24 + 3, 2 ** 24)) == F32(1.0 + 2.0 ** -22)     # a tie: to even, upwards
    assert wm.fl32(Fraction(0)) == F32(0.0)


def test_find_best_bin_edges():
    f = wm.find_best_bin
    # N / 2 <= 3: no k >= 2 with k + 1 < N / 2
    assert f(np.array([], F32)) is None and f(np.array([9, 9], F32)) is None
    assert f(np.array([0, 0, 5], F32)) is None
    # N / 2 = 4: only bin 2 can be chosen
    assert f(np.array([0, 0, 5, 1], F32)) == 2
    assert f(np.array([0, 0, 1, 5], F32)) is None                  # the maximum in the last bin can never be chosen
    # no crossing: every magnitude 0, nothing is above 0.8 * 0
    assert f(np.zeros(50, F32)) is None
    # a plateau is "still heading upwards" until it falls: the LAST bin of it
    assert f(np.array([0, 0, 1, 7, 7, 7, 2, 0], F32)) == 5
    assert f(np.array([0, 0, 1, 7, 7, 7, 7, 7], F32)) is None      # ... and never, when it reaches the end
    # the first bin above the threshold that falls, not the largest one
    assert f(np.array([0, 0, 1, 8.5, 3, 10, 2, 0], F32)) == 3
    assert f(np.array([0, 0, 1, 7.9, 3, 10, 2, 0], F32)) == 5      # 7.9 is not above 0.8f * 10
    # bins 0 and 1 are never looked at, neither for the maximum nor for the answer
    assert f(np.array([100, 100, 1, 2, 1, 0], F32)) == 3
    # the threshold is f32(0.8) * max in the vector's precision
    m = np.array([0, 0, F32(10.0) * F32(0.8), 1, 10, 0], F32)
    assert f(m) == 4 and f(m.astype(np.float64)) == 4
    assert f(np.array([0, 0, np.nextafter(F32(10.0) * F32(0.8), F32(100)), 1, 10, 0], F32)) == 2


def test_margin_agrees_with_find_best_bin():
    rng = np.random.default_rng(3)
    for _ in range(50):
        m = rng.uniform(0, 1, int(rng.integers(0, 40)))
        b, gap = wm.best_bin_margin(m)
        assert b == wm.find_best_bin(m) and gap >= 0


def test_builder_margin_on_the_seeds_the_gpu_tests_use():
    """the smallest gap of any comparison find_best_bin makes on the way to its answer is at least 0.01 C: the GPU tests leave
    out bursts whose margin is under 4 bound_spectrum (about 4e-6 C), so they leave out none of these"""
    worst = np.inf
    for seed in wm.GPU_SEEDS:
        x = wm.nrz_burst(seed)
        C = int(wm.pulses(x).sum())
        b, gap = wm.best_bin_margin(np.abs(wm.spectrum64(x)))
        assert b is not None and gap >= 0.01 * C, (seed, b, gap / C)
        assert gap > 4 * wm.bound_spectrum(C)
        worst = min(worst, gap / C)
    print(f"worst margin {worst:.4f} C")


def test_model_chain_recovers_a_g3ruh_frame():
    from bits_model import G3RUH, HDLC_FLAG, Chain
    x, tx = wm.g3ruh_burst(1)
    syms, tags, b, p0 = wm.process_one(x, samp_rate=50000.0)
    assert abs(len(x) / b - 5.2083) < 0.02 and tags["frequency"] == F32(tags["sps"] * F32(50000.0))
    bits, pos, diffs = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG).run(syms)
    assert wm.planted_offset(bits, tx) is not None


def test_process_one_drops_what_the_reference_drops():
    assert wm.process_one(np.ones(3, F32)) is None                 # n < 4
    assert wm.process_one(np.ones(100, F32)) is None               # no crossing
    assert wm.process_one(np.array([1, -1, 1, -1, 1, -1, 1, -1], F32)) is None      # N / 2 = 3
    assert wm.process_one(wm.nrz_burst(0), mid=float("nan")) is None


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ValueError, match="no usable HIP device"):
        rr.Wpcr()
