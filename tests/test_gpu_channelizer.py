"""The channelizer (rr_channelizer_create / rr_channelizer_u8_create): one shared input, N x {FftFilter(taps_c),
RationalResampler(I, D)} with Complex outputs.  Every channel must equal its own oracle chain
FftFilter(taps_c) -> RationalResampler(I, D) (src/fft_filter.rs:289-355, src/rational_resampler.rs:154-213) within the
plain 1e-5 bar, at the same length — on every kernel (decimate-first, half-size and full-size inverses) and on the
per-channel composition the constructor falls back to."""
import ctypes as C

import numpy as np
import pytest

from harness import WAIT_DST, WAIT_SRC, angle_parity, knob, max_norm_err, run_chain
from oracle import pyoracle as orc
from rustradio_amd import multi

pytestmark = pytest.mark.gpu
TOL = 1e-5
SB = 4_096_000


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


def sig(n, seed):
    """a few tones + noise, |x| ~ 1"""
    r = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.05 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for k, f in enumerate((0.003, -0.011, 0.047, 0.21)):
        x += np.exp(2j * np.pi * f * t + 1j * k) / 4
    return x.astype(np.complex64)


def chan_taps(proto, nchan):
    """the prototype shifted to nchan centres spread over the band"""
    k = np.arange(len(proto), dtype=np.float64)
    return np.stack([(proto.astype(np.complex128) * np.exp(2j * np.pi * (c / max(nchan, 1) - 0.5) * k)).astype(np.complex64)
                     for c in range(nchan)])


def drive(blk, x, nch, cap_in, cap_out, offset=0):
    """the reference's window protocol by hand -> ([nch] outputs, [(status, consumed, produced, need)])"""
    outs, log = [[] for _ in range(nch)], []
    pos, ring = 0, np.zeros(0, x.dtype)
    for _ in range(1_000_000):
        take = min(cap_in - len(ring), len(x) - pos)
        ring = np.concatenate([ring, x[pos:pos + take]]); pos += take
        if offset:                                   # a window at an odd byte address
            buf = np.zeros(len(ring) + offset, ring.dtype); buf[offset:] = ring
            win = buf[offset:]
        else:
            win = ring
        st, c, p, need, out = blk.work(win, cap_out)
        log.append((st, c, p, need))
        ring = ring[c:]
        out = out.reshape(nch, -1)
        for ch in range(nch):
            outs[ch].append(out[ch][:p])
        if take == 0 and c == 0 and p == 0:
            break
    else:
        raise AssertionError("no termination")
    return [np.concatenate(o) for o in outs], log


def check(yg, taps, I, D, x, sb=SB, pre=()):
    for ch in range(len(taps)):
        yo = run_chain(list(pre) + [orc.FftFilter(taps[ch]), orc.RationalResampler(I, D)], x, stream_bytes=sb)
        assert len(yg[ch]) == len(yo) > 0, (ch, len(yg[ch]), len(yo))
        assert max_norm_err(yg[ch], yo) <= TOL, (ch, max_norm_err(yg[ch], yo))


def cfg4():
    proto = orc.low_pass_complex(multi.CFG4_FS, 100e3, 12.5e3)
    return multi.cfg4_taps(proto, list(multi.shard_channels(32, 1, 0)))


def shape(name):
    """-> (taps [nchan][ntaps], I, D, n)"""
    if name == "cfg4-32ch-1:6":
        return cfg4(), 1, 6, 300_000
    if name.startswith("rtl-downsampled"):
        nch = int(name.split("-")[-1][:-2])
        return chan_taps(orc.low_pass_complex(250e3, 40e3, 1e3), nch), 1, 5, 250_000
    if name == "2467-taps-25:128":
        return chan_taps(orc.low_pass_complex(1.024e6, 100e3, 1e3), 2), 25, 128, 400_000
    if name == "463-taps-1:50":
        return cfg4()[:5], 1, 50, 300_000
    if name == "463-taps-1:200":
        return cfg4()[:3], 1, 200, 400_000
    if name == "400-taps-2:3":
        return chan_taps(orc.low_pass_complex(1e6, 100e3, 8e3)[:400], 3), 2, 3, 200_000
    if name == "3-taps-1:4":
        return chan_taps(np.array([0.25, 0.5 + 0.1j, 0.25], np.complex64), 2), 1, 4, 100_000
    if name.startswith("nchan-"):
        return cfg4()[:1].repeat(1, 0) if name == "nchan-1" else np.concatenate([cfg4()] * 2)[:int(name[6:])], 1, 6, 200_000
    raise KeyError(name)


SHAPES = ["cfg4-32ch-1:6", "rtl-downsampled-1ch", "rtl-downsampled-4ch", "2467-taps-25:128", "463-taps-1:50", "463-taps-1:200",
          "400-taps-2:3", "3-taps-1:4", "nchan-1", "nchan-2", "nchan-9", "nchan-33"]


@pytest.mark.parametrize("kernel", ["auto", "no-poly", "full"])
@pytest.mark.parametrize("name", SHAPES)
def test_channels_equal_their_oracle_chains(rr, monkeypatch, name, kernel):
    if kernel == "no-poly":
        knob(rr, monkeypatch, fm_poly=-1)
    elif kernel == "full":
        knob(rr, monkeypatch, fm_full=1)
    taps, I, D, n = shape(name)
    x = sig(n, len(taps) * 7 + D)
    blk = rr.Channelizer(taps, I, D)
    assert rr.lib().rr_block_out_windows(blk._h) == len(taps)
    assert "unfused" not in blk.name and "per channel" not in blk.name, blk.name
    yg, _ = drive(blk, x, len(taps), SB // 8, SB // 8)
    check(yg, taps, I, D, x)


def test_beyond_the_fused_kernels_runs_as_the_composition(rr):
    """5000 taps at 1:9: no fused kernel takes it (more than 4094 taps off the decimate-first tiles); the same constructor
    returns N x (FftFilter, RationalResampler) behind the handle, same protocol, same output"""
    taps = chan_taps(orc.low_pass_complex(1.024e6, 100e3, 500), 2)
    assert taps.shape[1] > 4094
    x = sig(200_000, 6)
    blk = rr.Channelizer(taps, 1, 9)
    assert "per channel" in blk.name, blk.name
    yg, _ = drive(blk, x, 2, SB // 8, SB // 8)
    check(yg, taps, 1, 9, x)


@pytest.mark.parametrize("kernel", ["auto", "full"])
def test_small_and_odd_windows(rr, monkeypatch, kernel):
    if kernel == "full":
        knob(rr, monkeypatch, fm_full=1)
    taps = cfg4()[:4]
    x = sig(250_000, 9)
    yg, log = drive(rr.Channelizer(taps, 1, 6), x, 4, 41_000, 30_000)
    assert any(st == WAIT_DST for st, *_ in log) or len(log) > 5
    check(yg, taps, 1, 6, x)


def _n2(y, I, D):
    return -(-y * I // D)


def model(S, I, D, calls):
    """the channelizer's work() protocol: FmMulti::work_blocks without the demodulator's lag"""
    n1, pend, out = 0, 0, []
    for in_len, cap in calls:
        nb = _n2(n1 + S, I, D) - _n2(n1, I, D)
        if nb > cap:
            out.append((WAIT_DST, 0, 0, nb)); continue
        total = pend + in_len
        k_in = total // S
        k_out = 0
        while _n2(n1 + (k_out + 1) * S, I, D) - _n2(n1, I, D) <= cap:
            k_out += 1
        if k_in > k_out:
            k = k_out; c = k * S - pend; pend = 0; st = WAIT_DST
            need = _n2(n1 + (k + 1) * S, I, D) - _n2(n1 + k * S, I, D)
        else:
            k = k_in; c = in_len; pend = total - k * S; st = WAIT_SRC; need = S - pend
        out.append((st, c, _n2(n1 + k * S, I, D) - _n2(n1, I, D), need))
        n1 += k * S
    return out


@pytest.mark.parametrize("I,D", [(1, 6), (2, 3), (25, 128)])
def test_protocol_is_the_n2_model(rr, I, D):
    taps = cfg4()[:2]
    S = orc.fftfilter_dims(orc.FftFilter(taps[0]))[1]
    blk = rr.Channelizer(taps, I, D)
    nb = _n2(S, I, D)
    x = sig(10 * S + 17, 3)
    calls = [(S - 5, 10_000), (40, nb - 1), (40, nb), (3 * S + 1, 2 * nb + 1), (0, 0), (2 * S, 10 * nb), (0, 10 * nb)]
    want = model(S, I, D, calls)
    pos = 0
    for (n_in, cap), w in zip(calls, want):
        st, c, p, need, _ = blk.work(x[pos:pos + n_in], cap)
        assert (st, c, p, need) == w, ((n_in, cap), (st, c, p, need), w)
        pos += c
    assert any(w[0] == WAIT_DST and w[1] == 0 for w in want) and any(w[0] == WAIT_SRC for w in want)


def test_output_window_at_and_below_the_threshold(rr):
    taps = cfg4()[:3]
    S = orc.fftfilter_dims(orc.FftFilter(taps[0]))[1]
    nb = _n2(S, 1, 6)
    x = sig(S, 4)
    st, c, p, need, _ = rr.Channelizer(taps, 1, 6).work(x, nb - 1)
    assert (st, c, p, need) == (WAIT_DST, 0, 0, nb)
    st, c, p, need, out = rr.Channelizer(taps, 1, 6).work(x, nb)
    assert (c, p) == (S, nb) and out.shape == (3, nb)
    for ch in range(3):
        yo = run_chain([orc.FftFilter(taps[ch]), orc.RationalResampler(1, 6)], x)
        assert max_norm_err(out[ch], yo[:nb]) <= TOL


@pytest.mark.parametrize("D,kernel", [(5, "auto"), (6, "auto"), (6, "full")])
def test_u8_source(rr, monkeypatch, D, kernel):
    if kernel == "full":
        knob(rr, monkeypatch, fm_full=1)
    taps = chan_taps(orc.low_pass_complex(2.4e6, 100e3, 12.5e3), 5)
    z = sig(200_000, D)
    b = np.empty(2 * len(z) + 1, np.uint8)                  # an odd byte count: the trailing byte is never consumed
    b[0:-1:2] = np.clip(np.round(z.real / 0.008 * 0.5 + 127), 0, 255).astype(np.uint8)
    b[1:-1:2] = np.clip(np.round(z.imag / 0.008 * 0.5 + 127), 0, 255).astype(np.uint8)
    b[-1] = 200
    x = run_chain([orc.RtlSdrDecode()], b)
    for off, cin in ((0, SB), (1, 40_001)):                  # even and odd-addressed windows, odd window sizes
        yg, _ = drive(rr.ChannelizerU8(taps, 1, D), b, 5, cin, SB // 8, offset=off)
        check(yg, taps, 1, D, x)


def test_device_resident_single_channel(rr):
    """nchan 1 between two HBM rings (rr_block_work_streams) = the same block on host windows"""
    taps = chan_taps(orc.low_pass_complex(250e3, 40e3, 1e3), 1)
    x = sig(300_000, 12)
    host, _ = drive(rr.Channelizer(taps, 1, 5), x, 1, SB // 8, SB // 8)
    blk = rr.Channelizer(taps, 1, 5)
    src, dst = rr.DeviceStream(np.complex64, SB), rr.DeviceStream(np.complex64, SB)
    pos, got = 0, []
    for _ in range(100_000):
        pos += src.push(x[pos:])
        st, c, p, need = blk.work_streams(src, dst)
        y = dst.pop()
        got.append(y)
        if c == 0 and p == 0 and len(y) == 0 and pos == len(x):
            break
    else:
        raise AssertionError("no termination")
    yg = np.concatenate(got)
    assert len(yg) == len(host[0]) > 1000 and np.array_equal(yg, host[0])


def _nan_poisoned(x, seed, extra=()):
    rng = np.random.default_rng(seed)
    x = x.copy()
    n = len(x)
    pos = sorted(set([0, 3, n // 7, n // 7 + 1, n // 3, n // 2 + 5, n - 9, n - 1] + [int(p) for p in rng.integers(0, n, 5)] + list(extra)))
    for k, p in enumerate(pos):
        x[p] = [complex(np.nan, 0.25), complex(-0.5, np.nan), complex(np.nan, np.nan)][k % 3]
    return x


@pytest.mark.parametrize("kind", ["poly", "poly-small", "full", "full-small", "half", "2:3"])
def test_nan_sets_are_the_references(rr, kind):
    """a NaN input sample makes exactly the reference's outputs NaN — the resampled samples of the FftFilter blocks it
    poisons, [b S, (b + 1) S + ntaps) (fft_filter.rs:326-347) — whatever GPU tile shared it; every other output is finite and
    within 1e-5 (csrc/kernels_misc.hip k_chan_blocks_nonfinite).  Small windows carry the verdicts across calls."""
    taps = np.stack([orc.low_pass_complex(2.4e6, 100e3, 12.5e3)] * 1)
    taps = np.concatenate([taps, np.conj(taps), (taps * np.exp(1j * 0.1 * np.arange(taps.shape[1]))).astype(np.complex64)])
    n, S = 400_000, 561
    x = _nan_poisoned(sig(n, 13), 13, extra=[(n // 2 // S) * S - 3, (n // 2 // S) * S + 2])
    I, D = (2, 3) if kind == "2:3" else (1, 6)
    opts = {"fm_poly": 8} if kind.startswith("poly") else {"fm_full": 1} if kind.startswith("full") else {"fm_poly": -1}
    with rr.build_options(**opts):
        blk = rr.Channelizer(taps, I, D)
    cap = 7_000 if "small" in kind else SB // 8
    yg, _ = drive(blk, x, 3, cap, cap)
    for ch in range(3):
        want = run_chain([orc.FftFilter(taps[ch]), orc.RationalResampler(I, D)], x)
        got = yg[ch]
        assert len(got) == len(want) > 1000
        bo = ~(np.isfinite(want.real) & np.isfinite(want.imag))
        bg = ~(np.isfinite(got.real) & np.isfinite(got.imag))
        assert 20 < bo.sum() < len(want)
        assert np.array_equal(bo, bg), (kind, ch, int(bo.sum()), int(bg.sum()), np.flatnonzero(bo != bg)[:8])
        assert max_norm_err(got[~bo], want[~bo]) <= TOL


def test_demodulated_channels_agree_with_fm_multi(rr):
    taps = cfg4()[:8]
    x = sig(300_000, 21)
    yc, _ = drive(rr.Channelizer(taps, 1, 6), x, 8, SB // 8, SB // 8)
    st, c, p, need, yf = rr.FmMulti(taps, 1, 6, 1.0).work(x, SB // 4)
    for ch in range(8):
        yd = run_chain([orc.QuadratureDemod(1.0)], yc[ch])
        m = min(len(yd), p)
        assert m > 10_000
        ro = run_chain([orc.FftFilter(taps[ch]), orc.RationalResampler(1, 6)], x)
        assert angle_parity(yf[ch][:m], yd[:m], ro[:m + 1])["used"] <= 1.0


def test_errors_and_tags(rr):
    taps = cfg4()[:2]
    for args, msg in (((taps, 1, 0), "RationalResampler created using deci 0"), ((taps, 0, 6), "RationalResampler created using interp 0"),
                      ((np.zeros((0, 463), np.complex64), 1, 6), "channel count"), ((np.zeros((4097, 3), np.complex64), 1, 6), "channel count"),
                      ((np.zeros((2, 0), np.complex64), 1, 6), "empty taps")):
        with pytest.raises(ValueError, match=msg):
            rr.Channelizer(*args)
        with pytest.raises(ValueError, match=msg):
            rr.ChannelizerU8(*args)
    for blk in (rr.Channelizer(taps, 1, 6), rr.ChannelizerU8(taps, 1, 6), rr.Channelizer(chan_taps(sig(5000, 1) / 1e3, 1), 1, 9)):
        p = C.c_size_t(0)
        assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == 0, blk.name      # RR_TAGS_DROP
    assert rr.lib().rr_abi_version() == 3


def test_zz_channelizer_create_work_destroy_soak(rr):
    """200 create -> work -> destroy cycles on fresh pageable windows, fused and composed; every cycle equals the first"""
    taps = cfg4()[:4]
    long_taps = chan_taps(orc.low_pass_complex(1.024e6, 100e3, 500), 2)
    x = sig(60_000, 31)
    first = {}
    for cycle in range(200):
        for key, t, D in (("fused", taps, 6), ("composed", long_taps, 9)):
            blk = rr.Channelizer(t, 1, D)
            xin = x.copy()
            st, c, p, need, out = blk.work(xin, 100_000)
            assert p > 1000
            if key not in first:
                first[key] = out.copy()
                yo = run_chain([orc.FftFilter(t[1]), orc.RationalResampler(1, D)], x)
                assert max_norm_err(out[1], yo[:p]) <= TOL
            else:
                assert np.array_equal(out, first[key]), (key, cycle)
            del blk, xin, out
