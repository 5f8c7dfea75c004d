"""rr_fm_receiver[_u8]_create — Tee + N x (FftFilter -> RationalResampler -> QuadratureDemod -> FftFilterFloat ->
RationalResampler -> MultiplyConst), examples/rtl_fm.rs:381-419 per channel — against the oracle's six blocks, channel by
channel, under the propagated bar of tests/receiver_model.py:

    bar[m] = |scale| (|audio_taps| * b)[q] + 1e-5 max|ref|        (b: harness.angle_parity's per-sample bound, tol 1e-5)

The first signals put ONE FM station in every channel's passband (conditions checked on the oracle in
test_fm_receiver_cpu.py): neighbouring channels' audio lies within a bar of each other there, so those tests cannot see a
receiver that confuses channels.  The distinct-station signals (receiver_model.shape_distinct: a station of its own per
channel, thousands of bars apart) carry the tests of the channel dimension: parity and the float64 truth of the whole chain,
every FmMulti kernel family, streaming with calls that only carry, silent channels that must stay exactly 0, NaN sets, the
three audio tiles with bit-identity to FmMulti + AudioChain, a switch of tile in mid-stream and a second fuzz family.
Also: the existing FmMulti + one AudioChain per channel as a twin, the window protocol against the Python model, page-locked
rings and device windows, NaN sets, launch counts, the shapes that run as a composition, constructor errors, fuzz and a soak."""
import ctypes as C

import numpy as np
import pytest

import receiver_model as rm
from harness import WAIT_DST, WAIT_SRC, drive_pageable, drive_registered, knob
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5
SB = 4_096_000


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


def mk(rr, sh, u8=False):
    f = rr.FmReceiverU8 if u8 else rr.FmReceiver
    return f(sh.taps, sh.rf[0], sh.rf[1], sh.audio_taps, sh.audio[0], sh.audio[1], sh.gain, sh.mode, sh.scale)


drive = rm.drive          # Graph::run's loop around the block (shared with the CPU test that runs it on the model alone)


def one_call(blk, x, nch):
    st, c, p, need, out = blk.work(x, 2_000_000)
    return list(np.atleast_2d(out))


def check_parity(yg, sh, x=None, chans=None, tag="", truth=False):
    """every channel against its oracle chain under the bar; prints the share of the bar used -> (worst share, oracle audio).
    truth: also against receiver_model.float64_truth under bar + |oracle - truth| per sample (the triangle inequality through
    the oracle, no tolerance of its own), the oracle's distance taken here"""
    worst, refs, worst_t, worst_o = 0.0, {}, 0.0, 0.0
    for ch in (range(sh.nchan) if chans is None else chans):
        au, dm, r = rm.oracle_channel(sh, ch, x)
        assert len(yg[ch]) == len(au) > 0, (sh.name, ch, len(yg[ch]), len(au))
        bar, plain = rm.audio_bar(sh, r, au)
        used = float(np.max(np.abs(yg[ch].astype(np.float64) - au.astype(np.float64)) / bar))
        assert used <= 1.0, (sh.name, tag, ch, used, int(np.argmax(np.abs(yg[ch].astype(np.float64) - au) / bar)))
        worst, refs[ch] = max(worst, used), au
        if truth:
            t = rm.float64_truth(sh, ch, len(au), x)
            dist = np.abs(au.astype(np.float64) - t)
            err = np.abs(yg[ch].astype(np.float64) - t) / (bar + dist)
            assert float(err.max()) <= 1.0, (sh.name, tag, ch, float(err.max()), int(np.argmax(err)))
            worst_t, worst_o = max(worst_t, float(err.max())), max(worst_o, float(np.max(dist / bar)))
    print(f"{sh.name} {tag}: at most {worst:.3f} of the propagated bar used over {len(refs)} channels"
          + (f"; against the float64 truth {worst_t:.3f} of bar + |oracle - truth| (the oracle itself {worst_o:.3f} of the bar)" if truth else ""))
    return worst, refs


def fused(rr, sh, u8=False):
    blk = mk(rr, sh, u8)
    assert "unfused" not in blk.name, (sh.name, blk.name)
    return blk


def source(sh, u8):
    """-> (what the block reads, the Complex stream the oracle reads)"""
    if not u8:
        return sh.x, sh.x
    b = rm.to_rtlsdr_bytes(sh.x)
    x = np.asarray(orc.RtlSdrDecode().work(b, len(b))[4])
    assert len(x) == len(sh.x)
    return b, x


# ---- parity against the oracle, every channel ---------------------------------------------------------------------------
def test_cfg4_like_32_channels(rr):
    sh = rm.shape_cfg4(nchan=32)
    yg, _ = drive(mk(rr, sh), sh.x, 32, [(SB // 8, SB // 4)])
    check_parity(yg, sh)


def test_rtl_fm_shape_4_channels(rr):
    sh = rm.shape_rtl_fm()
    yg, _ = drive(mk(rr, sh), sh.x, 4, [(SB // 8, SB // 4)])
    check_parity(yg, sh, truth=True)


SMALL = [(5, 65, (2, 3)), (50, 128, (7, 4)), (5, 1, (7, 4)), (50, 65, (2, 3)), (5, 128, (2, 3))]


@pytest.mark.parametrize("deci,audio_ntaps,audio", SMALL)
def test_small_odd_shapes(rr, deci, audio_ntaps, audio):
    """3 channels with distinct taps, RF decimations 5 and 50, audio filters of 1, 65 and 128 taps, audio ratios 2:3 and 7:4"""
    sh = rm.shape_small(deci, audio_ntaps, audio)
    yg, _ = drive(mk(rr, sh), sh.x, 3, [(SB // 8, SB // 4)])
    check_parity(yg, sh, truth=True)
    yg, log = drive(mk(rr, sh), sh.x, 3, [(7_001, 5_003), (20_011, 9_001)])
    assert sum(1 for *_, p, _n in log if p) >= 3
    check_parity(yg, sh, tag="small windows", truth=True)


@pytest.mark.parametrize("which", ["cfg4", "small"])
def test_u8_sources(rr, which):
    sh = rm.shape_cfg4(n=200_000, nchan=8) if which == "cfg4" else rm.shape_small(5, 65, (2, 3))
    b = rm.to_rtlsdr_bytes(sh.x)
    x = np.asarray(orc.RtlSdrDecode().work(b, len(b))[4])
    assert len(x) == len(sh.x)
    yg, log = drive(mk(rr, sh, u8=True), b, sh.nchan, [(SB, SB // 4)])
    check_parity(yg, sh, x=x, tag="u8")
    yg, log = drive(mk(rr, sh, u8=True), b, sh.nchan, [(30_001, 9_001)])       # odd byte windows, odd addresses after a consume
    check_parity(yg, sh, x=x, tag="u8 odd windows")


@pytest.mark.parametrize("kernel", ["w8", "w12", "full", "half"])
def test_forced_rf_kernels(rr, monkeypatch, kernel):
    opts = {"w8": dict(fm_poly=8), "w12": dict(fm_poly=12), "full": dict(fm_full=1, fm_poly=-1), "half": dict(fm_poly=-1)}[kernel]
    knob(rr, monkeypatch, **opts)
    sh = rm.shape_cfg4(n=200_000, nchan=8)
    yg, _ = drive(mk(rr, sh), sh.x, 8, [(SB // 8, SB // 4)])
    check_parity(yg, sh, tag=kernel)


def test_one_channel(rr):
    sh = rm.shape_cfg4(n=200_000, nchan=1)
    blk = mk(rr, sh)
    assert rr.lib().rr_block_out_windows(blk._h) == 1
    yg, _ = drive(blk, sh.x, 1, [(SB // 8, SB // 4)])
    check_parity(yg, sh)


# ---- the twin: the existing FmMulti, then one existing AudioChain per channel --------------------------------------------
@pytest.mark.parametrize("which", ["cfg4", "rtl_fm", "small"])
def test_twin_fm_multi_plus_audio_chains(rr, which):
    """the same input through rr.FmMulti and one rr.AudioChain per channel — unchanged code, each held to the oracle elsewhere.
    The new block must agree to the plain 1e-5 max|ref|: no atan2 amplification between the two, they demodulate alike."""
    sh = {"cfg4": lambda: rm.shape_cfg4(n=200_000, nchan=8), "rtl_fm": lambda: rm.shape_rtl_fm(n=300_000),
          "small": lambda: rm.shape_small(5, 65, (2, 3))}[which]()
    ya = one_call(mk(rr, sh), sh.x, sh.nchan)
    st, c, p, need, dm = rr.FmMulti(sh.taps, sh.rf[0], sh.rf[1], sh.gain, sh.mode).work(sh.x, 2_000_000)
    dm = np.atleast_2d(dm)
    identical = True
    for ch in range(sh.nchan):
        st, c, p, need, yb = rr.AudioChain(sh.audio_taps, sh.audio[0], sh.audio[1], sh.scale).work(dm[ch], 2_000_000)
        assert len(ya[ch]) == len(yb) > 1000, (ch, len(ya[ch]), len(yb))
        err = float(np.max(np.abs(ya[ch].astype(np.float64) - yb)) / np.max(np.abs(yb)))
        assert err <= TOL, (which, ch, err)
        identical = identical and np.array_equal(ya[ch].view(np.uint32), yb.view(np.uint32))
    print(f"twin {which}: bit-identical to FmMulti + AudioChain: {identical}")


# ---- streaming: the log is the Python model's, the output the one-call output -------------------------------------------
def _stream_cases():
    cases = []
    for i, (deci, ant, audio) in enumerate([(5, 65, (2, 3)), (50, 128, (7, 4)), (5, 1, (7, 4)), (5, 128, (2, 3))]):
        for j, u8 in enumerate((False, True)):
            cases.append((deci, ant, audio, u8, "mixed"))
            cases.append((deci, ant, audio, u8, "short-in"))
        cases.append((deci, ant, audio, False, "tight-out"))
    return cases


@pytest.mark.parametrize("deci,ant,audio,u8,kind", _stream_cases())
def test_streaming_log_is_the_model(rr, deci, ant, audio, u8, kind):
    """a dozen or more emitting calls on odd windows: input windows shorter than S1, output windows below the next step
    (WAIT_DST consuming nothing) and between steps (WAIT_DST after k_out blocks).  (status, consumed, produced, need) of
    every call equal the model's; the stream equals the one-call output within the bar (tiles start where calls start, so the
    rounding differs) and the oracle's."""
    m = rm.ReceiverModel(len(orc.low_pass_complex(1e6, 0.35e6 / deci, 0.15e6 / deci)), 1, deci, ant, *audio, u8=u8)
    n = max(40 * m.S1, 30 * m.S2 * deci) + 17                     # 30 audio blocks at least
    sh = rm.shape_small(deci, ant, audio, n=n)
    assert sh.model(u8).S1 == m.S1
    S1 = m.S1 * (2 if u8 else 1)
    step = max(m.A(k + 1) - m.A(k) for k in range(n // m.S1))
    if kind == "mixed":
        caps = [(3 * S1 + 7, 2 * step + 3), (S1 // 2 + 1, step - 1), (5 * S1 + 1, step), (S1 + 3, 6 * step + 1)]
    elif kind == "short-in":
        caps = [(S1 // 3 + 1, 4 * step + 5), (S1 // 2 + 2, 4 * step + 5), (2 * S1 + 1, 4 * step + 5)]
    else:
        caps = [(9 * S1 + 5, step), (9 * S1 + 5, step // 2), (9 * S1 + 5, 2 * step + 1)]
    xs = sh.x
    src = rm.to_rtlsdr_bytes(xs) if u8 else xs
    x = np.asarray(orc.RtlSdrDecode().work(src, len(src))[4]) if u8 else xs
    yg, log = drive(mk(rr, sh, u8), src, 3, caps)
    want = [(st, c, p, need) for st, c, p, need in (m.work(cin, cout) for cin, cout, *_ in log)]
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]
    assert sum(1 for st, c, p, need in got if p) >= 12, sum(1 for st, c, p, need in got if p)
    if kind == "tight-out":                   # both WAIT_DST forms: nothing consumed, and k_out blocks consumed
        assert any(st == WAIT_DST and c == 0 and p == 0 for st, c, p, need in got)
        assert any(st == WAIT_DST and c > 0 for st, c, p, need in got)
    elif kind == "mixed":
        assert any(st == WAIT_DST for st, c, p, need in got)
    else:
        assert sum(1 for i, *_ in log if 0 < i < S1) >= len(log) // 2          # input windows shorter than one RF block
    assert any(st == WAIT_SRC for st, c, p, need in got)
    _, refs = check_parity(yg, sh, x=x, tag=f"{kind} u8={u8}")
    once = one_call(mk(rr, sh, u8), src, 3)
    for ch in range(3):
        au, dm, r = rm.oracle_channel(sh, ch, x)
        bar, _ = rm.audio_bar(sh, r, au)
        assert len(once[ch]) == len(yg[ch])
        assert np.all(np.abs(once[ch].astype(np.float64) - yg[ch]) <= bar), (kind, ch)


# ---- page-locked rings and device windows -------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=["c32", "u8"])
def test_registered_rings(rr, u8):
    sh = rm.shape_small(5, 65, (2, 3))
    m = sh.model(u8)
    src = rm.to_rtlsdr_bytes(sh.x) if u8 else sh.x
    x = np.asarray(orc.RtlSdrDecode().work(src, len(src))[4]) if u8 else sh.x
    cin = (4 * m.S1 + 3) * (2 if u8 else 1) | 1
    cout = 3 * max(m.A(k + 1) - m.A(k) for k in range(64)) + 1
    ya, la = drive_pageable(mk(rr, sh, u8), src, cin, cout)
    yb, lb = drive_registered(rr, mk(rr, sh, u8), src, cin, cout)
    assert la == lb and sum(1 for st, c, p, need in lb if p) >= 4
    assert ya.shape == yb.shape
    check_parity(list(yb), sh, x=x, tag="registered")
    check_parity(list(ya), sh, x=x, tag="pageable")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("nchan", [2, 9])
def test_device_windows(rr, nchan, off):
    """rr_block_work_dev on device windows an odd out_cap apart, starting at element 0 or 1: the host-window log, the
    host-window samples bit for bit, and not one element behind `produced` in any channel window touched"""
    import torch
    sh = rm.shape_small(5, 65, (2, 3), nchan=nchan, n=60_000)
    m = sh.model()
    cin, cout = 6 * m.S1 + 5, (4 * max(m.A(k + 1) - m.A(k) for k in range(64))) | 1
    x = sh.x
    host, hlog = drive(mk(rr, sh), x, nchan, [(cin, cout)])
    blk = mk(rr, sh)
    dx = torch.from_numpy(x.view(np.float32).copy()).cuda()
    total = off + nchan * cout + 5
    sentinel = np.full(total, np.float32(-7777.25), np.float32)
    dy = torch.from_numpy(sentinel.copy()).cuda()
    fill = dy.clone()
    got, log, pos = [[] for _ in range(nchan)], [], 0
    for _ in range(10_000):
        in_len = min(cin, len(x) - pos)
        dy.copy_(fill)
        torch.cuda.synchronize()
        st, c, p, need = blk.work_dev(dx.data_ptr() + 8 * pos, in_len, dy.data_ptr() + 4 * off, cout)
        blk.sync()
        y = dy.cpu().numpy()
        log.append((st, c, p, need))
        untouched = np.ones(total, bool)
        for ch in range(nchan):
            lo = off + ch * cout
            got[ch].append(y[lo:lo + p].copy())
            untouched[lo:lo + p] = False
        assert np.array_equal(y[untouched].view(np.uint32), sentinel[untouched].view(np.uint32)), (nchan, off, len(log), p)
        pos += c
        if in_len == len(x) - pos + c and c == 0 and p == 0:
            break
    else:
        raise AssertionError("no termination")
    assert log == [(st, c, p, need) for _i, _o, st, c, p, need in hlog][:len(log)] and sum(1 for st, c, p, need in log if p) >= 4
    for ch in range(nchan):
        yd = np.concatenate(got[ch])
        assert len(yd) == len(host[ch]) > 1000 and np.array_equal(yd.view(np.uint32), host[ch].view(np.uint32)), (nchan, off, ch)


# ---- NaN sets -----------------------------------------------------------------------------------------------------------
NAN_WHERE = ["block-edge", "call-end", "call-start", "middle"]


def _nan_case(rr, sh, where):
    nchan = sh.nchan
    m = sh.model()
    cin = 7 * m.S1 + 11
    cout = 4 * max(m.A(k + 1) - m.A(k) for k in range(64)) + 1
    pos = {"block-edge": 9 * m.S1 - 1, "call-end": 2 * cin - 1, "call-start": 2 * cin, "middle": 20 * m.S1 + m.S1 // 2}[where]
    x = sh.x.copy()
    x[pos] = complex(np.nan, 0.25)
    yg, log = drive(mk(rr, sh), x, nchan, [(cin, cout)])
    for ch in range(nchan):
        au, dm, r = rm.oracle_channel(sh, ch, x)
        assert len(yg[ch]) == len(au)
        bo, bg = ~np.isfinite(au), ~np.isfinite(yg[ch])
        assert 10 < bo.sum() < len(au)
        assert np.array_equal(bo, bg), (where, nchan, ch, int(bo.sum()), int(bg.sum()), np.flatnonzero(bo != bg)[:8])
        # the bar from the clean stream's |r| (the poisoned stretch has none)
        au0, dm0, r0 = rm.oracle_channel(sh, ch)
        bar, _ = rm.audio_bar(sh, r0, au0)
        ok = ~bo
        assert np.all(np.abs(yg[ch][ok].astype(np.float64) - au[ok]) <= bar[ok]), (where, nchan, ch)


@pytest.mark.parametrize("nchan", [2, 9])
@pytest.mark.parametrize("where", NAN_WHERE)
def test_nan_sets_are_the_references(rr, nchan, where):
    """one NaN input sample: at an RF block edge, as the last sample of a call, as the first of the next, mid-block.  It
    poisons its RF block (fft_filter.rs:326-347), the resampled and demodulated samples of that block, and the audio blocks
    those fall in: the set of non-finite audio outputs is exactly the oracle's, finite outputs stay within the bar."""
    _nan_case(rr, rm.shape_small(5, 65, (2, 3), nchan=nchan, n=60_000), where)


@pytest.mark.parametrize("where", NAN_WHERE)
def test_nan_sets_with_distinct_stations(rr, where):
    """the same four positions on five channels with a station each: the non-finite pass refolds the smeared samples around a
    poisoned block channel by channel, from that channel's window and verdict slots — another channel's are thousands of bars off"""
    sh = rm.distinct("5x5-65")
    assert "unfused" not in mk(rr, sh).name
    _nan_case(rr, sh, where)


# ---- launch count -------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_nchan(rr):
    """a clean emitting call: two tile kernels and two non-finite passes on a Complex source, two tile kernels on bytes"""
    counts = {}
    for nchan in (4, 32):
        sh = rm.shape_cfg4(n=120_000, nchan=nchan)
        for u8 in (False, True):
            blk = mk(rr, sh, u8)
            src = rm.to_rtlsdr_bytes(sh.x) if u8 else sh.x
            half = len(src) // 2 // 2 * 2
            blk.work(src[:half], SB // 4)                                     # first call: buffers grow, state settles
            before = rr.lib().rr_debug_kernel_launches()
            st, c, p, need, out = blk.work(src[half:], SB // 4)
            counts[(nchan, u8)] = rr.lib().rr_debug_kernel_launches() - before
            assert p > 1000 and np.all(np.isfinite(out))
    print("launches per clean emitting call:", counts)
    assert counts[(4, False)] == counts[(32, False)] <= 4
    assert counts[(4, True)] == counts[(32, True)] <= 2


# ---- shapes beyond the fused kernels: the composition behind the same handle ---------------------------------------------
@pytest.mark.parametrize("kind", ["audio-4000", "rf-5000", "fastfm"])
def test_composition_shapes(rr, kind):
    """more than 3584 audio taps, RF filters FmMulti runs per channel, FastFM: whole-stream equality with the oracle chain
    (the window protocol is the composition's own: only progress and termination are asked of it)"""
    if kind == "audio-4000":
        sh = rm.shape_small(5, 65, (2, 3), n=120_000)
        sh.audio_taps = rm.sinc_low_pass(4000, 0.1)
    elif kind == "rf-5000":
        sh = rm.shape_small(5, 65, (2, 3), n=120_000)
        fs = 1e6
        proto = rm.sinc_low_pass(5000, 0.07).astype(np.complex64)
        sh.taps = rm.shifted(proto, fs, [-1e4, 0.0, 1e4])
        sh.skip = 5000 // 5 + 2
    else:
        sh = rm.shape_small(5, 65, (2, 3), mode=rm.DEMOD_FASTFM)
    blk = mk(rr, sh)
    assert "unfused" in blk.name, blk.name
    yg, log = drive(blk, sh.x, 3, [(SB // 8, SB // 4)])
    assert sum(1 for *_, p, _n in log if p) >= 1
    for ch in range(3):
        au, dm, r = rm.oracle_channel(sh, ch)
        assert len(yg[ch]) == len(au) > 1000, (kind, ch, len(yg[ch]), len(au))
        if kind == "fastfm":                  # no atan2: the plain bound on the whole chain
            assert float(np.max(np.abs(yg[ch].astype(np.float64) - au)) / np.max(np.abs(au))) <= 10 * TOL, (kind, ch)
        else:
            bar, _ = rm.audio_bar(sh, r, au)
            assert np.all(np.abs(yg[ch].astype(np.float64) - au) <= bar), (kind, ch)
    yg2, log2 = drive(mk(rr, sh), sh.x, 3, [(9_001, 1_001), (30_011, 4_001)])
    assert [len(y) for y in yg2] == [len(y) for y in yg]


# ---- constructor errors -------------------------------------------------------------------------------------------------
def test_constructor_errors_and_tags(rr):
    sh = rm.shape_small(5, 65, (2, 3), n=1000)
    t, a = sh.taps, sh.audio_taps
    bad = [((t, 1, 0, a, 2, 3), "RationalResampler created using deci 0"), ((t, 0, 5, a, 2, 3), "RationalResampler created using interp 0"),
           ((t, 1, 5, a, 2, 0), "RationalResampler created using deci 0"), ((t, 1, 5, a, 0, 3), "RationalResampler created using interp 0"),
           ((np.zeros((0, 65), np.complex64), 1, 5, a, 2, 3), "channel count"), ((np.zeros((4097, 3), np.complex64), 1, 5, a, 2, 3), "channel count"),
           ((np.zeros((2, 0), np.complex64), 1, 5, a, 2, 3), "empty taps"), ((t, 1, 5, np.zeros(0, np.float32), 2, 3), "empty taps")]
    for args, msg in bad:
        for f in (rr.FmReceiver, rr.FmReceiverU8):
            with pytest.raises(ValueError, match=msg):
                f(*args)
    for blk in (mk(rr, sh), mk(rr, sh, u8=True)):
        p = C.c_size_t(0)
        assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == 0, blk.name      # RR_TAGS_DROP
        assert rr.lib().rr_block_out_windows(blk._h) == 3
        assert blk.eof(True) and not blk.eof(False)
    assert rr.lib().rr_abi_version() == 3


# ---- distinct stations: every channel hears a station no other channel hears ---------------------------------------------
ODD = [(7_001, 5_003), (20_011, 9_001)]


def _windows(u8):
    return ([(SB, SB // 4)], [(30_001, 9_001)]) if u8 else ([(SB // 8, SB // 4)], ODD)


@pytest.mark.parametrize("key", ["4x10", "9x10", "5x5", "32x40", "5x6-2.4M", "9x10-u8", "5x5-u8"])
def test_distinct_stations_parity_and_truth(rr, key):
    """4 and 9 channels at 1:10, 5 at 1:5, 32 at 1:40, 5 at 1:6 from 2.4 Msps (the decimate-first tiles of six phases), RTL-SDR
    bytes: every channel within the bar of its own oracle chain and of the float64 truth, in ring-sized and in odd windows"""
    sh, u8 = rm.distinct(key), key.endswith("u8")
    src, x = source(sh, u8)
    ring, odd = _windows(u8)
    yg, _ = drive(fused(rr, sh, u8), src, sh.nchan, ring)
    check_parity(yg, sh, x=x, tag=key, truth=True)
    yg, log = drive(fused(rr, sh, u8), src, sh.nchan, odd)
    assert sum(1 for *_, p, _n in log if p) >= 3
    check_parity(yg, sh, x=x, tag=key + " odd windows", truth=True)


@pytest.mark.parametrize("kernel", ["w8", "w12", "full", "half"])
def test_forced_rf_kernels_with_distinct_stations(rr, monkeypatch, kernel):
    """test_forced_rf_kernels' four choices at its tap count and ratio (463 taps, 1:6 from 2.4 Msps), five stations apart"""
    opts = {"w8": dict(fm_poly=8), "w12": dict(fm_poly=12), "full": dict(fm_full=1, fm_poly=-1), "half": dict(fm_poly=-1)}[kernel]
    knob(rr, monkeypatch, **opts)
    sh = rm.distinct("5x6-2.4M-463")
    assert sh.taps.shape[1] == 463
    yg, _ = drive(fused(rr, sh), sh.x, 5, [(SB // 8, SB // 4)])
    check_parity(yg, sh, tag=kernel, truth=True)
    yg, log = drive(fused(rr, sh), sh.x, 5, ODD)
    assert sum(1 for *_, p, _n in log if p) >= 3
    check_parity(yg, sh, tag=kernel + " odd windows", truth=True)


@pytest.mark.parametrize("kind", rm.STREAM_KINDS)
@pytest.mark.parametrize("key", ["5x5", "5x5-u8", "9x10-400", "9x10-400-u8"])
def test_streaming_distinct_stations(rr, key, kind):
    """test_streaming_log_is_the_model's three kinds of windows on 5 and 9 channels with a station each: the log is the model's,
    a dozen emitting calls, the stream within the bar of the oracle and of the one-call output.  The 400-tap audio filter takes
    624 demodulated samples per block where an RF block brings 35: most calls there only carry (k_audio_multi_carry) — counted
    from the model's lengths (test_fm_receiver_cpu.py runs this loop on the model alone and asserts the same counts)."""
    sh, u8 = rm.distinct(key), key.endswith("u8")
    src, x = source(sh, u8)
    caps = rm.stream_caps(sh.model(u8), kind, len(sh.x))
    yg, log = drive(fused(rr, sh, u8), src, sh.nchan, caps)
    m = sh.model(u8)
    want = [m.work(cin, cout) for cin, cout, *_ in log]
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]
    assert sum(1 for st, c, p, need in got if p) >= 12, sum(1 for st, c, p, need in got if p)
    assert any(st == WAIT_SRC for st, c, p, need in got)
    if kind != "short-in":
        assert any(st == WAIT_DST for st, c, p, need in got)
    lens = rm.call_lengths(sh.model(u8), log)
    carry_only = sum(1 for k, dm, ny, p in lens if dm > 0 and ny == 0)
    print(f"{key} {kind}: {len(log)} calls, {sum(1 for *_, p in lens if p)} emitting, {carry_only} that only carry")
    if "400" in key:
        assert carry_only >= 12, carry_only
    _, refs = check_parity(yg, sh, x=x, tag=f"{key} {kind}", truth=True)
    once = one_call(fused(rr, sh, u8), src, sh.nchan)
    for ch in range(sh.nchan):
        au, dm, r = rm.oracle_channel(sh, ch, x)
        bar, _ = rm.audio_bar(sh, r, au)
        assert len(once[ch]) == len(yg[ch])
        assert np.all(np.abs(once[ch].astype(np.float64) - yg[ch]) <= bar), (key, kind, ch)


@pytest.mark.parametrize("mode", [rm.ATAN2_EXACT, rm.ATAN2_FAST], ids=["exact", "fast"])
@pytest.mark.parametrize("nchan,live", [(3, 0), (3, 1), (3, 2), (9, 0), (9, 4), (9, 8)])
def test_silent_channels_stay_exactly_zero(rr, nchan, live, mode):
    """one channel with its RF taps, all others with zero taps, every station on the air: a zero-tap channel's resampled samples
    are 0, their angle is 0 in both atan2 forms, the audio is 0 (the oracle's is, checked here and without a GPU).  Over a
    stream of many calls every sample of every silent channel must be == 0 — anything that crosses a stride, a carry row or a
    mid row shows as a non-zero sample, no bar involved — and the live channel stays within its bar."""
    sh = rm.shape_distinct(nchan, 10, live=live, mode=mode)
    yg, log = drive(fused(rr, sh), sh.x, nchan, ODD)
    assert sum(1 for *_, p, _n in log if p) >= 6
    for ch in range(nchan):
        if ch == live:
            continue
        au, dm, r = rm.oracle_channel(sh, ch)
        assert len(au) == len(yg[ch]) > 1000 and np.all(au == 0), (nchan, live, ch)
        nz = np.flatnonzero(yg[ch] != 0)
        assert len(nz) == 0, (nchan, live, ch, len(nz), nz[:8], yg[ch][nz[:4]])
    check_parity(yg, sh, chans=[live], tag=f"live {live} of {nchan} mode {mode}")


@pytest.mark.parametrize("lg,key", [(10, "9x10"), (11, "5x10-400"), (12, "9x10-900")])
def test_forced_audio_tiles_and_bit_identity(rr, monkeypatch, lg, key):
    """k_audio_multi<10>, <11> and <12> by name (rr_build_opts.fft_log2f; 65, 400 and 900 audio taps), stations apart: parity
    in ring-sized and odd windows.  A forced tile leaves the block without its second, smaller tile, so what DESIGN 4.8 says
    must hold: one call of the receiver is bit for bit FmMulti followed by one AudioChain per channel (same options)."""
    knob(rr, monkeypatch, fft_log2f=lg)
    sh = rm.distinct(key)
    assert len(sh.audio_taps) + 1 <= 1 << lg
    yg, _ = drive(fused(rr, sh), sh.x, sh.nchan, [(SB // 8, SB // 4)])
    check_parity(yg, sh, tag=f"tile 2^{lg}", truth=True)
    yg, log = drive(fused(rr, sh), sh.x, sh.nchan, ODD)
    assert sum(1 for *_, p, _n in log if p) >= 3
    check_parity(yg, sh, tag=f"tile 2^{lg} odd windows", truth=True)
    ya = one_call(fused(rr, sh), sh.x, sh.nchan)
    st, c, p, need, dm = rr.FmMulti(sh.taps, sh.rf[0], sh.rf[1], sh.gain, sh.mode).work(sh.x, 2_000_000)
    dm = np.atleast_2d(dm)
    for ch in range(sh.nchan):
        st, c, p, need, yb = rr.AudioChain(sh.audio_taps, sh.audio[0], sh.audio[1], sh.scale).work(dm[ch], 2_000_000)
        assert len(ya[ch]) == len(yb) > 1000, (ch, len(ya[ch]), len(yb))
        diff = np.flatnonzero(ya[ch].view(np.uint32) != yb.view(np.uint32))
        assert len(diff) == 0, (lg, key, ch, len(diff), diff[:8], float(np.max(np.abs(ya[ch] - yb))))


def test_audio_tile_switches_in_mid_stream(rr):
    """9 channels, 400 audio taps: the block holds the 2048-point tile (by cost) and the 1024-point one for calls whose
    channels x tiles are fewer than the CUs.  Windows of 2.3 M and 0.15 M samples alternate: by the model's lengths every large
    call has C ceil(n_y / (2 (4096 - L + 1))) >= CUs (the large tile whichever the first tile is) and every small one
    C ceil(n_y / (2 (1024 - L + 1))) < CUs (the small tile whichever).  The carry, the history and the verdict slots pass from
    one tile's launch to the other's: the log is the model's, every channel within the bar.  (That both k_audio_multi<11> and
    <10> run here is in profiles/fm_receiver_probe.md, from a kernel trace of this test.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sh = rm.distinct("9x10-400", n=5_000_000)
    C, L = sh.nchan, len(sh.audio_taps)
    caps = [(2_300_000, 400_000), (150_000, 400_000)]
    yg, log = drive(fused(rr, sh), sh.x, C, caps)
    m = sh.model()
    want = [m.work(cin, cout) for cin, cout, *_ in log]
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]
    kinds = []
    for k, dm, ny, p in rm.call_lengths(sh.model(), log):
        if ny:
            large = C * -(-ny // (2 * (4096 - L + 1))) >= cus
            small = C * -(-ny // (2 * (1024 - L + 1))) < cus
            assert large != small, (ny, cus)
            kinds.append("L" if large else "s")
    print(f"tile switch: {cus} CUs, emitting calls {''.join(kinds)}")
    assert "".join(kinds).count("Ls") >= 2 and "".join(kinds).count("sL") >= 1, kinds
    check_parity(yg, sh, tag="tile switch", truth=True)


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_distinct_stations(rr, seed):
    """2 to 17 channels with a station each, integer RF decimations, audio taps, ratios and windows as test_fuzz draws them,
    Complex or bytes: never the composition, the log is the model's, every channel within the bar"""
    sh, u8, caps = rm.fuzz_distinct(seed)
    src, x = source(sh, u8)
    yg, log = drive(fused(rr, sh, u8), src, sh.nchan, caps)
    m = sh.model(u8)
    want = [m.work(cin, cout) for cin, cout, *_ in log]
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert got == want, (seed, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:3])
    assert sum(1 for st, c, p, need in got if p) >= 2
    check_parity(yg, sh, x=x, tag=f"fuzz-distinct {seed} u8={u8} caps={caps}")


# ---- seeded fuzz --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(rr, seed):
    """tap counts, ratios, channel counts and windowing drawn from the seed; the log is the model's, every channel within the bar"""
    g = np.random.default_rng(1000 + seed)
    deci = int(g.choice([2, 3, 5, 6, 8, 10, 25]))
    rf_interp = int(g.choice([1, 1, 1, 2, 3]))
    if rf_interp >= deci or np.gcd(rf_interp, deci) != 1:
        rf_interp = 1
    ant = int(g.choice([1, 2, 17, 64, 65, 200, 511]))
    audio = [(2, 3), (7, 4), (1, 1), (3, 25), (6, 25), (1, 4), (4, 2)][int(g.integers(0, 7))]
    nchan = int(g.choice([1, 2, 3, 5, 9]))
    u8 = bool(g.integers(0, 2))
    sh = rm.shape_small(deci, ant, audio, nchan=nchan, rf_interp=rf_interp, seed=seed, n=int(g.integers(50_000, 90_000)))
    m = sh.model(u8)
    S1 = m.S1 * (2 if u8 else 1)
    step = max(max(m.A(k + 1) - m.A(k) for k in range(200)), 1)
    caps = [(int(g.integers(S1 // 3 + 1, 6 * S1)), int(g.integers(max(step // 2, 1), 5 * step + 2))) for _ in range(3)] + [(4 * S1 + 1, 3 * step + 1)]
    src = rm.to_rtlsdr_bytes(sh.x) if u8 else sh.x
    x = np.asarray(orc.RtlSdrDecode().work(src, len(src))[4]) if u8 else sh.x
    yg, log = drive(mk(rr, sh, u8), src, nchan, caps)
    want = [m.work(cin, cout) for cin, cout, *_ in log]
    got = [(st, c, p, need) for _i, _o, st, c, p, need in log]
    assert got == want, (seed, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:3])
    check_parity(yg, sh, x=x, tag=f"fuzz {seed} nchan={nchan} u8={u8} caps={caps}")


# ---- soak ---------------------------------------------------------------------------------------------------------------
def test_zz_create_work_destroy_soak(rr):
    """200 create -> work -> destroy cycles, fused and composed; every cycle equals the first"""
    fused = rm.shape_small(5, 65, (2, 3), n=40_000)
    comp = rm.shape_small(5, 65, (2, 3), n=40_000, mode=rm.DEMOD_FASTFM)
    first = {}
    for cycle in range(200):
        for key, sh in (("fused", fused), ("composed", comp)):
            blk = mk(rr, sh)
            st, c, p, need, out = blk.work(sh.x.copy(), 100_000)
            assert p > 1000
            if key not in first:
                first[key] = out.copy()
            else:
                assert np.array_equal(out.view(np.uint32), first[key].view(np.uint32)), (key, cycle)
            del blk, out
