"""GPU: the device paths of rr_symbol_sync (kernels_sync.hip) that tests/test_gpu_symsync.py does not reach — tap counts other than
2 with a clock that moves, sps just above 1 and at 200, 2,048 and 4,096 streams with a gather that strides more than once, windows
that grow under several streams, positions beyond 2^20 and a non-finite clock — against the sequential machine of
tests/symsync_model.py.  Every comparison is bit for bit (uint32 views, equal counts, equal state); only the NaNs of the non-finite
case are compared as NaNs, and that test says why.  Each test asserts on the model the property that makes it non-vacuous.  Every
input shape here first passes symsync_core.hpp under g++ in tests/test_symsync_cpu.py."""
import functools

import numpy as np
import pytest

import rustradio_amd as rr
import symsync_model as sm
from symsync_dev import dev_push, u32

pytestmark = pytest.mark.gpu


def handle(prm, nstreams=1, lanes=None):
    if lanes is None:
        return rr.SymbolSync(*prm, nstreams=nstreams)
    with rr.build_options(sync_lanes=lanes):
        h = rr.SymbolSync(*prm, nstreams=nstreams)
    assert h.streams_per_wave == lanes
    return h


def run_and_compare(h, rows, prm, pushes, strides=None, equal=sm.states_equal):
    """the rows (one per stream of h) through h and through one model each, push by push: counts, symbols, clock values and the
    state of every stream after every push -> the models"""
    rows = np.atleast_2d(rows)
    models = [sm.SymbolSync(*prm) for _ in rows]
    at = 0
    for n in pushes:
        ist, ost = (n, n) if strides is None else (n + strides[0], n + strides[1])
        counts, syms, clk = dev_push(h, rows[:, at:at + n], in_stride=ist, out_stride=ost)
        for c, m in enumerate(models):
            ws, wc, _ = m.run(rows[c, at:at + n])
            assert counts[c] == len(ws), (n, c)
            assert np.array_equal(u32(syms[c]), u32(ws)) and np.array_equal(u32(clk[c]), u32(wc)), (n, c)
            assert equal(h.state(c), m.state()), (n, c)
        at += n
    assert at == rows.shape[1]
    return models


# ---- 1. tap counts ----------------------------------------------------------------------------------------------------------------------
TAPS = {"1": (0.5, [0.25]), "3": (0.5, [0.2, 0.5, 0.3]), "5": (0.5, [0.1, 0.4, 0.2, 0.2, 0.1]),
        "8": (0.5, [0.05, 0.3, 0.2, 0.15, 0.1, 0.08, 0.07, 0.05]), "8-wide": (2.5, [0.3, 0.3, 0.2, 0.1, 0.05, 0.03, 0.01, 0.01])}
TAPS_N = 2490


@functools.lru_cache(maxsize=None)
def taps_rows():
    """5 distinct rows of 500 noisy symbols at sps 5, each with a clock offset of its own"""
    x = np.stack([sm.nrz(500, 5.0, 23 + c, offset=0.004 - 0.002 * c, smooth=1 + c % 3, noise=0.2)[:TAPS_N] for c in range(5)])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("layout", [(1, None), (5, 1), (5, 64)], ids=["one-stream", "5-streams-1-lane", "5-streams-64-lanes"])
@pytest.mark.parametrize("key", list(TAPS))
def test_tap_counts_with_a_moving_clock(key, layout):
    """1, 3, 5 and 8 taps: the unrolled accumulation and history shift of sync_filter_clamped as the device builds them (mul_rn /
    add_rn under -ffp-contract=fast), hist included in the compared state.  On the model: more than 200 clock updates per row, more
    than 100 distinct clock bit patterns where the filter has a history, fewer than half of the clock values at a clamp limit."""
    dev, taps = TAPS[key]
    prm = (5.0, dev, taps)
    nstreams, lanes = layout
    rows = taps_rows()[:nstreams]
    models = run_and_compare(handle(prm, nstreams, lanes), rows, prm, (1237, TAPS_N - 1237))
    for c, m in enumerate(models):
        clk = sm.SymbolSync(*prm).run(rows[c])[1]
        assert m.clock_updates > 200, c
        assert len(taps) == 1 or len(set(u32(clk).tolist())) > 100, c
        assert np.mean((clk == np.float32(5.0 - dev)) | (clk == np.float32(5.0 + dev))) < 0.5, c
        assert len(m.state()["hist"]) == len(taps) - 1


# ---- 2. sps edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(sm.SPS_EDGES))
def test_sps_edges(key):
    """sps 1.25 and the smallest f32 above 1: nearly every sample is a symbol and the output window nearly full; sps 200: a handful
    of emissions.  3,000 samples in pushes of 1, 63, 64, 65, 0 and the rest."""
    prm = sm.SPS_EDGES[key]
    x = sm.sps_edge_signal(key)
    assert len(x) == sm.SPS_EDGE_N == 3000 and sm.SPS_EDGE_PUSHES[:5] == (1, 63, 64, 65, 0)
    total = len(sm.SymbolSync(*prm).run(x)[0])
    if key in ("1.25", "1+ulp"):
        assert total >= 0.99 * len(x)
    if key == "200":
        assert 10 <= total <= 20
    if key == "1+ulp":
        assert np.float32(prm[0]) > 1 and np.float32(prm[0]) - np.float32(1) == np.float32(2.0 ** -23)
    run_and_compare(handle(prm), x, prm, sm.SPS_EDGE_PUSHES, strides=(3, 5))


# ---- 3. 2,048 and 4,096 streams: the gather strides more than once -------------------------------------------------------------------------
MANY_PRM, MANY_N = sm.SPS_EDGES["1.25"], 700


@functools.lru_cache(maxsize=None)
def base_rows():
    """8 distinct rows of 765 samples and the model's answer for each in pushes of 700 and 65 -> (samples, [per push (symbols,
    clock values)], [state after the second push])"""
    x = np.stack([sm.nrz(640, MANY_PRM[0], 300 + b, offset=0.002 * (b - 3), noise=0.1)[:MANY_N + 65] for b in range(8)])
    assert x.shape == (8, MANY_N + 65)
    want, states = [], []
    for b in range(8):
        m = sm.SymbolSync(*MANY_PRM)
        want.append([m.run(x[b, :MANY_N])[:2], m.run(x[b, MANY_N:])[:2]])
        states.append(m.state())
    x.setflags(write=False)
    return x, want, states


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("nstreams", [2048, 4096])
def test_many_streams_and_the_second_pass_of_the_gather(nstreams, lanes):
    """k_sync_gather gives a row min(ceil(n / 256), max(1, 8 CUs / nstreams)) workgroups of 256 threads: with more than 512
    emissions per row (asserted on the model) at 2,048 streams or more, a row's workgroups stride at least twice for any CU count
    up to 512.  Row c is base row (5 c + nstreams) % 8, so the model runs 8 times."""
    x, want, states = base_rows()
    assert all(len(w[0][0]) > 512 for w in want)
    assert len({len(w[0][0]) for w in want}) > 1                       # (the rows differ in their counts too)
    pick = [(5 * c + nstreams) % 8 for c in range(nstreams)]
    h = handle(MANY_PRM, nstreams, lanes)
    for push, (lo, hi) in enumerate(((0, MANY_N), (MANY_N, MANY_N + 65))):
        # dev_push fills the outputs with sentinels and asserts that every element behind a row's count still holds one
        counts, syms, clk = dev_push(h, x[pick, lo:hi], in_stride=hi - lo + 3, out_stride=hi - lo + 5)
        for c in range(nstreams):
            ws, wc = want[pick[c]][push]
            assert counts[c] == len(ws), (push, c)
            assert np.array_equal(u32(syms[c]), u32(ws)) and np.array_equal(u32(clk[c]), u32(wc)), (push, c)
    for c in sorted({0, 1, 63, 64, 65, 2047, nstreams - 1}):
        assert sm.states_equal(h.state(c), states[pick[c]]), c


# ---- 4. windows that grow under several streams ------------------------------------------------------------------------------------------
def test_growing_windows_with_several_streams():
    """idx and words are indexed c n and c nwords and reserved again when n grows: pushes of 64, 1,000, 65, 3,000 and 1 samples
    through one handle of 5 streams, strides n + 3 and n + 5"""
    pushes = (64, 1000, 65, 3000, 1)
    n = sum(pushes)
    prm = sm.ADAPTIVE_9600
    rows = np.stack([sm.nrz(n // 5 + 8, prm[0], 400 + c, offset=((c * 5) % 13 - 6) * 0.0007, smooth=1 + c % 4, noise=0.05 + 0.03 * c)[:n]
                     for c in range(5)])
    assert rows.shape == (5, n)
    models = run_and_compare(handle(prm, 5), rows, prm, pushes, strides=(3, 5))
    assert all(m.clock_updates > 300 for m in models)
    assert len({u32(sm.SymbolSync(*prm).run(r)[0]).tobytes() for r in rows}) == 5


# ---- 5. positions beyond 2^20 --------------------------------------------------------------------------------------------------------------
GAP, GAP_AT = (1 << 20) + 1000, 600


@functools.lru_cache(maxsize=None)
def long_gap():
    """stream 0: GAP zeros in front of sample 600 of a noisy signal; streams 1 and 2: ordinary signals of the same length.  The
    signal of stream 0 holds 1,400 symbols, not 400: behind the gap the positions come down by one step-back (10 clock, about 52)
    per SAMPLE, so 400 symbols (2,083 samples) cannot show more than 1,500 of them (measured: 1,498), and the condition of more
    than 5,000 step-backs at positions where an ulp is 1/8 is kept instead of the shorter signal.
    -> (samples [3, n], [(symbols, clock values, state)] per row, the model of row 0, its clock updates up to the end of the gap)"""
    prm = sm.ADAPTIVE_9600
    sig = sm.nrz(1400, prm[0], 31, offset=0.002, smooth=3, noise=0.05)
    x0 = sm.with_gap(sig, GAP_AT, GAP)
    n = len(x0)
    rows = np.stack([x0] + [sm.nrz(n // 5 + 8, prm[0], 32 + c, offset=0.003 * c - 0.004, smooth=3, noise=0.1)[:n] for c in (1, 2)])
    want, models = [], []
    for r in rows:
        m = sm.SymbolSync(*prm)
        s, c, _ = m.run(r)
        want.append((s, c, m.state()))
        models.append(m)
    before = sm.SymbolSync(*prm)
    before.run(x0[:GAP_AT + GAP])
    rows.setflags(write=False)
    return rows, want, models[0], before.clock_updates


@pytest.mark.parametrize("lanes", [1, 64])
def test_a_run_past_2_to_the_20_samples_without_a_sign_change(lanes):
    """stream_pos passes 2^20, where `+ 1.0` and `+ clock` round at 1/8: the fold loop runs about 200,000 times at the first sign
    change behind the gap, then the positions step back thousands of times while the clock goes on updating.  Under the 64-lane
    mapping the two ordinary streams share the wave with that loop."""
    rows, want, m0, updates_before = long_gap()
    assert m0.max_fold_iters > 150_000 and m0.step_backs > 5000 and m0.clock_updates - updates_before >= 100
    # the signal in front of and behind the gap is recovered: the signs of symbols 20 to 100 (behind the clock's start-up) and of the last 1,000 are runs of
    # the levels that were sent (sm.nrz draws them first from its seed), and the gap itself comes out as zeros
    s0 = want[0][0]
    sent = bytes(np.random.default_rng(31).integers(0, 2, 1400).astype(np.uint8))
    assert bytes((s0[20:100] > 0).astype(np.uint8)) == sent[20:100] and bytes((s0[-1000:] > 0).astype(np.uint8)) in sent[300:]
    assert not s0[200:-1400].any()
    h = handle(sm.ADAPTIVE_9600, 3, lanes)
    counts, syms, clk = dev_push(h, rows)
    for c in range(3):
        ws, wc, wstate = want[c]
        assert counts[c] == len(ws), c
        assert np.array_equal(u32(syms[c]), u32(ws)) and np.array_equal(u32(clk[c]), u32(wc)), c
        assert sm.states_equal(h.state(c), wstate), c


# ---- 6. the non-finite clock ---------------------------------------------------------------------------------------------------------------
def test_non_finite_clock_emits_nothing_more():
    """taps [1.0, 3e38, -3e38]: the first clock update adds +Inf and -Inf, f32::clamp hands the NaN through, and with a NaN clock
    and next_sym_middle no sample is a symbol any more: 5 symbols come out of 1,500 samples (both `while` conditions of sync_step are false on NaN, so the lane ends).
    Symbols, clock values and counts are compared bit for bit; the fields of state() that are NaN on the model must be NaN on the
    device, compared by isnan and not by payload: IEEE 754 leaves the payload and sign of a NaN that an operation makes to the
    implementation (numpy on x86 gives 0xffc00000), so its bits are no property of the block."""
    prm, x = sm.NONFINITE, sm.nonfinite_signal()
    m = sm.SymbolSync(*prm)
    syms, _, idx = m.run(x)
    st = m.state()
    assert len(x) == 1500 and len(syms) == 5 and idx.max() < 64 and m.clock_updates >= 1
    assert np.isnan(st["clock"]) and np.isnan(st["next_sym_middle"]) and np.isnan(st["hist"]).all() and st["stream_pos"] == 1500.0
    for pushes in ((1500,), (700, 800)):
        h = handle(prm)
        run_and_compare(h, x, prm, pushes, equal=sm.states_match)
        got = h.state(0)
        assert np.isnan(got["clock"]) and np.isnan(got["hist"]).all() and len(got["hist"]) == 2
