"""No GPU: the conditions the receive-chain tests of tests/test_gpu_rx_chain.py rely on, asserted on the models alone
(symsync_model.SymbolSync -> hdlcrx_helpers.ModelReceiver, and a float64 front end for the FM band).  They are properties of the
signals of tests/rx_chain_helpers.py, not of the code under test: with them the bit-for-bit equalities of the GPU tests are not
vacuous."""
import numpy as np

import rx_chain_helpers as rc
import symsync_model as sm

ORDINARY = [c for c in range(rc.RAGGED_N) if c not in (rc.ZERO_ROW, rc.GAP_ROW, rc.SPECIALS_ROW)]


def delivered(model, c):
    return [f[1] for push in model for f in push["frames"][c]]


def test_ragged_signal_every_ordinary_row_recovers_its_three_payloads():
    m = rc.ragged_model()
    assert len(m) == 3 and len(ORDINARY) == 63
    for c in ORDINARY:
        assert delivered(m, c) == rc.ragged_payloads(c), c
        assert m[-1]["stats"][c] == (3, 0, 0) and not any(f[2] for push in m for f in push["frames"][c]), c
    # the all-zero row emits symbols at the free-running clock and no frame
    assert m[-1]["consumed"][rc.ZERO_ROW] > 1500 and delivered(m, rc.ZERO_ROW) == [] and all(p["counts"][rc.ZERO_ROW] > 0 for p in m)
    # 3,000 zeros inside the second frame: that frame is lost, the third is recovered
    want = rc.ragged_payloads(rc.GAP_ROW)
    assert delivered(m, rc.GAP_ROW) == [want[0], want[2]]
    # NaN, +-Inf and +-0.0 sprinkled in: symbols still come in every push
    assert all(p["counts"][rc.SPECIALS_ROW] > 0 for p in m)
    x = rc.ragged_samples()
    assert np.isnan(x[rc.SPECIALS_ROW]).any() and np.isinf(x[rc.SPECIALS_ROW]).any() and not x[rc.ZERO_ROW].any()


def test_ragged_signal_counts_differ_between_streams_in_every_push():
    """What a receiver that read counts[0] for every stream, or a clock kernel that wrote a count to a neighbour's slot, cannot
    pass.  The streams lock to 13 clock offsets within +-0.42 %, so the number of distinct counts a push CAN show grows with its
    length: about 534 symbols (first push) spread over 6 values, 1,050 (third) over many; a push of 64 samples at a clock within
    [4.71, 5.71] holds 11 to 14 symbols whatever the stream, and shows 2 values.  Measured on the models: 6, 2 and 20 distinct
    counts among the first 64 streams.  Stream 64 differs from stream 0 in every push; stream 65 has stream 0's clock offset
    (((5 c) % 13 is 0 for both) and differs from it where its longer frames do, in the third."""
    m = rc.ragged_model()
    distinct = [len(set(p["counts"][:64])) for p in m]
    print("distinct counts per push among the first 64 streams:", distinct)
    assert distinct[0] >= 6 and distinct[1] >= 2 and distinct[2] >= 8
    for p, pairs in zip(m, (30, 8, 30)):
        assert p["counts"][64] != p["counts"][0]
        # neighbouring streams differ (the offsets step by 5 of 13 from stream to stream): in about half of the 65 pairs where a
        # push shows many values, and in 8 at least where it can only show two
        assert sum(p["counts"][c] != p["counts"][c + 1] for c in range(65)) >= pairs
    assert m[2]["counts"][65] != m[2]["counts"][0]
    assert len(set(m[-1]["consumed"])) >= 20
    # the second wave of the 64-lane mapping is partly filled, and its streams are ordinary ones
    assert rc.RAGGED_N == 66 and 64 in ORDINARY and 65 in ORDINARY


def test_ragged_signal_a_frame_straddles_each_push_boundary():
    """a frame delivered behind a boundary whose first bit lies in front of it: its end position less its unstuffed length
    (an upper bound of where it began) is below the symbols consumed up to the boundary"""
    m = rc.ragged_model()
    for i in (0, 1):
        hit = [c for c in ORDINARY for push in m[i + 1:] for f in push["frames"][c]
               if f[0] - 8 * (len(f[1]) + 2) < m[i]["consumed"][c] <= f[0]]
        assert hit, i


def test_ragged_signal_with_flipped_bits_is_repaired_in_three_streams():
    m, plain = rc.ragged_model(rc.FIX), rc.ragged_model()
    for c in range(rc.RAGGED_N):
        if c in rc.FLIPPED_ROWS:
            assert m[-1]["stats"][c] == (3, 0, 1) and delivered(m, c) == rc.ragged_payloads(c), c
            assert sum(f[2] for push in m for f in push["frames"][c]) == 1
        else:
            assert m[-1]["stats"][c] == plain[-1]["stats"][c] and delivered(m, c) == delivered(plain, c), c
    # without HDLC_FIX_BITS the same copy loses those frames
    x = rc.ragged_samples(True)
    lost = rc.chain_model(x[list(rc.FLIPPED_ROWS)], rc.ragged_cuts(x.shape[1]), rc.RAGGED_PRM, (1, rc.RAGGED_MAX_SIZE),
                          dict(nrzi=True, descrambler=rc.G3RUH))
    assert [s[0] for s in lost[-1]["stats"]] == [2, 2, 2]


def test_fm_signal_through_a_float64_front_end():
    """All 15 packets come back through convolution, every tenth sample and the angle of r[m + 1] conj(r[m]) in float64, then the two
    models; and the device's front end may differ from the oracle's by harness.angle_parity's bound without moving a symbol across
    0: from symbol 100 (inside the opening flags, behind the filter's start-up) to the end of the last frame the smallest |symbol|
    of a channel is at least 100 times the largest per-sample bound there.  Measured: the smallest |symbol| is 0.083 (channel 3;
    0.089, 0.49, 0.49 and 0.62 in the others), the bound 5.3e-5 in every channel — a factor of 1,500 at least."""
    taps = rc.fm_taps()
    assert taps.shape == (5, 129) and len(rc.fm_samples()) > 70_000
    for ch in range(rc.FM_NCHAN):
        dm, r = rc.fm_front_end_f64(ch)
        row = dm.astype(np.float32)
        m = rc.fm_model([row], [len(row)])[0]
        assert [f[1] for f in m["frames"][0]] == rc.fm_payloads(ch) and m["stats"][0] == (3, 0, 0), ch
        assert 1500 < m["counts"][0] < 1600
        syms, _, idx = sm.SymbolSync(*rc.FM_PRM).run(row)
        span = slice(100, m["frames"][0][-1][0])
        smallest, bound = float(np.abs(syms[span]).min()), float(rc.angle_bound(r)[idx[span]].max())
        print(f"channel {ch}: smallest |symbol| {smallest:.3g}, bound {bound:.3g}, ratio {smallest / bound:.0f}")
        assert smallest >= 100 * bound, ch
