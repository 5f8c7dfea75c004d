"""CPU-only checks behind tests/test_gpu_fm_receiver.py: the Python protocol model A(k) against the oracle's six blocks, the
conditions the parity signals must meet (checked on the oracle alone), the oracle's distance from the float64 statement of
the whole chain, the same conditions plus the separation of the channels for the distinct-station signals (and the record of
why those exist: the shared-station signals cannot tell neighbours apart), the streaming tests' windows on the model alone, and
the names of the new entry points in the header, the ctypes list and the Rust extern block."""
import os
import re

import numpy as np
import pytest

import receiver_model as rm
from harness import run_chain
from oracle import pyoracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(L1, rf, L2, audio, fastfm):
    t1 = (np.hanning(L1 + 2)[1:-1] / max(L1 / 2, 1)).astype(np.complex64)
    t2 = rm.sinc_low_pass(L2, 0.2)
    dem = orc.FastFM() if fastfm else orc.QuadratureDemod(1.0)
    return [orc.FftFilter(t1), orc.RationalResampler(*rf), dem, orc.FftFilterFloat(t2),
            orc.RationalResampler(*audio, dtype=np.float32), orc.MultiplyConst(0.5)]


# (rf taps, rf ratio, audio taps, audio ratio, FastFM, stream length): interp above and below 1 in both stages, both demodulators,
# a stream shorter than one RF block, one shorter than one audio block, unreduced ratios
PROTOCOL_SHAPES = [
    (463, (1, 6), 241, (3, 25), False, 300_000),
    (2467, (25, 128), 963, (6, 25), False, 200_000),
    (65, (1, 5), 65, (2, 3), False, 50_001),
    (65, (1, 5), 65, (2, 3), True, 50_001),
    (31, (3, 2), 1, (7, 4), False, 20_000),
    (31, (3, 2), 128, (7, 4), True, 20_000),
    (803, (1, 50), 64, (1, 1), False, 400_000),
    (100, (2, 4), 100, (6, 4), False, 77_777),
    (463, (1, 6), 241, (3, 25), False, 300),          # shorter than one RF block
    (463, (1, 6), 2000, (3, 25), False, 9_000),       # RF blocks, but less than one audio block
    (463, (1, 6), 241, (3, 25), True, 561 * 7),
]


@pytest.mark.parametrize("L1,rf,L2,audio,fastfm,n", PROTOCOL_SHAPES)
def test_protocol_model_counts_what_the_six_blocks_emit(L1, rf, L2, audio, fastfm, n):
    x = (np.random.default_rng(n).standard_normal(n) + 1j).astype(np.complex64)
    y = run_chain(_chain(L1, rf, L2, audio, fastfm), x)
    m = rm.ReceiverModel(L1, *rf, L2, *audio, fastfm=fastfm)
    assert len(y) == m.A(n // m.S1), (len(y), m.A(n // m.S1), m.S1, m.S2)
    if n < m.S1 or m.d(n // m.S1 * m.S1) < m.S2:
        assert len(y) == 0
    # ... and the model driven call by call ends on the same total, whatever the windows
    done = pos = have = 0
    cap = max(m.A(k + 1) - m.A(k) for k in range(n // m.S1 + 1)) + 7        # holds the largest single step, little more
    for _ in range(100_000):
        take = min(5 * m.S1 // 3 - have, n - pos)
        have += take; pos += take
        st, c, p, need = m.work(have, cap)
        have -= c; done += p
        if take == 0 and c == 0 and p == 0:
            break
    assert done == len(y)


def parity_shapes():
    return [rm.shape_cfg4(nchan=32), rm.shape_rtl_fm(), rm.shape_small(5, 65, (2, 3)), rm.shape_small(50, 128, (7, 4)),
            rm.shape_small(5, 1, (7, 4))]


@pytest.mark.parametrize("idx", range(5))
def test_parity_signals_meet_the_conditions_and_the_float64_truth(idx):
    """every parity signal, on the oracle alone: max |angle| <= 0.9 pi and min |r| >= 0.1 max |r| behind the RF start-up in
    every channel; at most 2 % of a channel's audio samples carry a bar above 10 x the plain term; and the oracle's distance
    from the float64 truth of the whole chain, in units of the bar and — away from the start-up samples, where |r| is small and
    the bar wide — of max |truth| (printed; profiles/fm_receiver_probe.md)"""
    sh = parity_shapes()[idx]
    worst_ang, worst_mag, worst_share, worst_truth, worst_rel = 0.0, 1.0, 0.0, 0.0, 0.0
    chans = range(sh.nchan) if sh.nchan <= 4 else (0, sh.nchan // 2, sh.nchan - 1)
    for ch in chans:
        au, dm, r = rm.oracle_channel(sh, ch)
        assert len(au) > 1000, (sh.name, ch, len(au))
        ang, mag = rm.signal_conditions(dm, r, sh.skip)
        assert ang <= 0.9 * np.pi and mag >= 0.1, (sh.name, ch, ang / np.pi, mag)
        bar, plain = rm.audio_bar(sh, r, au)
        share = float(np.mean(bar > 10 * plain))
        assert share <= 0.02, (sh.name, ch, share)
        truth = rm.float64_truth(sh, ch, len(au))
        err = np.abs(au.astype(np.float64) - truth)
        worst_truth, worst_rel = max(worst_truth, float(np.max(err / bar))), max(worst_rel, float(err[bar <= 10 * plain].max() / np.max(np.abs(truth))))
        worst_ang, worst_mag, worst_share = max(worst_ang, ang / np.pi), min(worst_mag, mag), max(worst_share, share)
    print(f"{sh.name}: max|angle| {worst_ang:.3f} pi, min|r|/max|r| {worst_mag:.3f}, {100 * worst_share:.2f} % of samples with bar > 10 x plain; "
          f"oracle vs float64 truth: {worst_truth:.3f} of the bar; {worst_rel:.2e} of max|truth| "
          f"where the bar is within 10 x plain")


@pytest.mark.parametrize("key", sorted(rm.DISTINCT))
def test_distinct_station_signals_meet_the_conditions_and_are_apart(key):
    """every distinct-station signal, on the oracle alone, in EVERY channel: the three conditions of the shared-station signals
    (max |angle| <= 0.9 pi, min |r| >= 0.1 max |r|, at most 2 % of the samples with a bar above 10 x plain), the oracle within
    the bar of the float64 truth, and the power of the GPU tests that use them: for every ordered pair of channels the median
    over samples (behind the start-up tenth) of |au_c - au_c'| / bar_c is at least 100.  That last one is a condition, not a
    measurement: a receiver that confuses two channels anywhere cannot stay within the bar."""
    sh, u8 = rm.distinct(key), key.endswith("u8")
    x = None
    if u8:
        b = rm.to_rtlsdr_bytes(sh.x)
        x = np.asarray(orc.RtlSdrDecode().work(b, len(b))[4])
    au, bar = {}, {}
    w_ang, w_mag, w_share, w_truth = 0.0, 1.0, 0.0, 0.0
    for ch in range(sh.nchan):
        au[ch], dm, r = rm.oracle_channel(sh, ch, x)
        assert len(au[ch]) > 1000, (sh.name, ch, len(au[ch]))
        ang, mag = rm.signal_conditions(dm, r, sh.skip)
        assert ang <= 0.9 * np.pi and mag >= 0.1, (sh.name, ch, ang / np.pi, mag)
        bar[ch], plain = rm.audio_bar(sh, r, au[ch])
        share = float(np.mean(bar[ch] > 10 * plain))
        assert share <= 0.02, (sh.name, ch, share)
        truth = rm.float64_truth(sh, ch, len(au[ch]), x)
        used = float(np.max(np.abs(au[ch].astype(np.float64) - truth) / bar[ch]))
        assert used <= 1.0, (sh.name, ch, used)
        w_ang, w_mag, w_share, w_truth = max(w_ang, ang / np.pi), min(w_mag, mag), max(w_share, share), max(w_truth, used)
    lo = len(au[0]) // 10
    meds = []
    for c in range(sh.nchan):
        for d in range(sh.nchan):
            if c != d:
                med = float(np.median(np.abs(au[c][lo:].astype(np.float64) - au[d][lo:]) / bar[c][lo:]))
                assert med >= 100.0, (sh.name, c, d, med)
                meds.append(med)
    print(f"{sh.name} u8={u8}: max|angle| {w_ang:.3f} pi, min|r|/max|r| {w_mag:.3f}, {100 * w_share:.2f} % of samples with bar > 10 x plain; "
          f"oracle vs float64 truth: {w_truth:.3f} of the bar; median neighbour distance {min(meds):.0f} - {max(meds):.0f} bars over {len(meds)} pairs")


def test_shared_station_signals_cannot_tell_neighbours_apart():
    """why the distinct-station signals exist: on the cfg4 signal (one station in every passband) a channel's oracle audio lies
    within its neighbour's bar in every sample — printed, with the 1-bar line asserted for the 8-channel form most tests used"""
    sh = rm.shape_cfg4(n=200_000, nchan=8)
    dist = rm.neighbour_distance(sh)
    worst = max(mx for (c, d), (med, mx, within) in dist.items() if abs(c - d) == 1)
    print(f"cfg4 x 8: neighbouring channels differ by at most {worst:.2f} bars")
    assert worst < 1.0, worst
    for args in ((5, 65, (2, 3)), (50, 128, (7, 4))):
        s3 = rm.shape_small(*args)
        d3 = [v for (c, d), v in rm.neighbour_distance(s3).items() if abs(c - d) == 1]
        print(f"{s3.name}: neighbours median {min(v[0] for v in d3):.1f} - {max(v[0] for v in d3):.1f} bars, max {max(v[1] for v in d3):.0f}, "
              f"{100 * max(v[2] for v in d3):.0f} % of samples within the bar")


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_distinct_signals_are_valid_and_apart(seed):
    """the second fuzz family's draws, on the oracle alone: no wrap flip can reach the audio filter (0.9 pi, 0.1) and every pair of
    channels is at least 100 bars apart in the median.  (Not the 2 % line: these streams are short on purpose, their start-up
    stretch is a larger share; the bar is wide there, not wrong.)"""
    sh, u8, caps = rm.fuzz_distinct(seed)
    assert sh.nchan <= sh.rf[1] and len(caps) == 4
    x = None
    if u8:
        b = rm.to_rtlsdr_bytes(sh.x)
        x = np.asarray(orc.RtlSdrDecode().work(b, len(b))[4])
    for ch in range(sh.nchan):
        au, dm, r = rm.oracle_channel(sh, ch, x)
        ang, mag = rm.signal_conditions(dm, r, sh.skip)
        assert len(au) > 100 and ang <= 0.9 * np.pi and mag >= 0.1, (seed, sh.name, ch, len(au), ang / np.pi, mag)
    worst = min(v[0] for v in rm.neighbour_distance(sh, x=x).values())
    print(f"fuzz-distinct {seed}: {sh.name} u8={u8}, channels at least {worst:.0f} bars apart in the median")
    assert worst >= 100.0, (seed, sh.name, worst)


@pytest.mark.parametrize("kind", rm.STREAM_KINDS)
@pytest.mark.parametrize("key", ["5x5", "5x5-u8", "9x10-400", "9x10-400-u8"])
def test_streaming_windows_reach_what_the_gpu_test_says(key, kind):
    """test_streaming_distinct_stations' loop on the protocol model alone: a dozen emitting calls, both waits, and — with 400
    audio taps — a dozen calls in which demodulated samples arrive but no whole audio block does (the carry-only launch)"""
    nchan, deci, ant, audio, kw = rm.DISTINCT[key]
    u8 = key.endswith("u8")
    rf_ntaps = len(orc.low_pass_complex(1e6, 0.35e6 / deci, 0.15e6 / deci))
    n = int(deci * max(8000, 60 * ant))
    mk_model = lambda: rm.ReceiverModel(rf_ntaps, 1, deci, ant, *audio, u8=u8)
    src = np.zeros(2 * n, np.uint8) if u8 else np.zeros(n, np.complex64)
    _, log = rm.drive(rm.ModelBlock(mk_model(), nchan), src, nchan, rm.stream_caps(mk_model(), kind, n))
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert sum(1 for st, c, p, need in got if p) >= 12
    assert any(st == rm.WAIT_SRC for st, c, p, need in got)
    assert kind == "short-in" or any(st == rm.WAIT_DST for st, c, p, need in got)
    lens = rm.call_lengths(mk_model(), log)
    assert sum(p for *_, p in lens) == mk_model().A(n // mk_model().S1)
    carry_only = sum(1 for k, dm, ny, p in lens if dm > 0 and ny == 0)
    assert "400" not in key or carry_only >= 12, carry_only


@pytest.mark.parametrize("mode", [rm.ATAN2_EXACT, rm.ATAN2_FAST])
def test_a_zero_tap_channel_is_exactly_silent_on_the_oracle(mode):
    """what test_silent_channels_stay_exactly_zero holds the GPU to: zero RF taps -> audio == 0 (values; the sign of a zero may vary)"""
    sh = rm.shape_distinct(3, 10, live=1, mode=mode)
    for ch in (0, 2):
        au, dm, r = rm.oracle_channel(sh, ch)
        assert len(au) > 1000 and np.all(r == 0) and np.all(dm == 0) and np.all(au == 0), (mode, ch)
    au, dm, r = rm.oracle_channel(sh, 1)
    assert np.max(np.abs(au)) > 0.5


def test_new_entry_points_are_named_everywhere():
    hdr = open(os.path.join(ROOT, "include", "rustradio_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    ext = re.search(r'unsafe extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    from rustradio_amd._lib import SYMBOLS
    for name in ("rr_fm_receiver_create", "rr_fm_receiver_u8_create"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in SYMBOLS, name
        assert re.search(r"fn\s+" + name + r"\s*\(", ext), name
    assert "pub struct GpuFmReceiver" in rust
    import rustradio_amd as rr
    assert callable(rr.FmReceiver) and callable(rr.FmReceiverU8)
    host = open(os.path.join(ROOT, "rustradio_amd", "host", "rustradio.hpp")).read()
    assert "class FmReceiver" in host and "rr_fm_receiver_create" in host
