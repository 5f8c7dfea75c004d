"""The channelizer (rr_channelizer_create / rr_channelizer_u8_create): one shared input, N x {FftFilter(taps_c),
RationalResampler(I, D)} with Complex outputs.  Every channel must equal its own oracle chain
FftFilter(taps_c) -> RationalResampler(I, D) (src/fft_filter.rs:289-355, src/rational_resampler.rs:154-213) within the
plain 1e-5 bar, at the same length — on every kernel (decimate-first, half-size and full-size inverses) and on the
per-channel composition the constructor falls back to."""
import ctypes as C
import math

import numpy as np
import pytest

from harness import (AGAIN, WAIT_DST, WAIT_SRC, angle_parity, drive_pageable, drive_registered, knob, max_norm_err,
                     resampled_filter_truth, run_chain)
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


def drive(blk, x, nch, cap_in, cap_out, offset=0, calls=None):
    """the reference's window protocol by hand -> ([nch] outputs, [(status, consumed, produced, need)]); `calls` collects
    every call's (input length, output window)"""
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
        if calls is not None:
            calls.append((len(win), cap_out))
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


# ---- streaming state, kernel edges, caller-owned windows: against the oracle AND the float64 statement ------------------
def nsamples(L):
    """FftFilter's block (fft_filter.rs:36-42, 261-262)"""
    n = 1
    while n < L:
        n <<= 1
    return 2 * n - L


def expected_kernel(L, I, D, opts=None):
    """FmMulti::FmMulti's path selection for the channelizer (csrc/blocks.cpp) -> "poly" (decimate-first
    tiles), "half" / "full" (shared-forward tiles, half-size / full-size inverse) or "per channel" (the composition):
    decimate-first for a reduced ratio 1:2 .. 1:8 at up to 768 taps per phase unless fm_poly < 0 or fm_full; else the
    shared-forward tiles of the cheapest of 1024 / 2048 / 4096 points (FftFilter's fitted tile costs, fft_log2f forces one)
    for up to 4095 taps, refused where ceil(D / I) >= F - L + 1; the half-size inverse on 2048-point tiles for 1:even with
    ((2048 - L + 1) - D - 1) / 2 > 0 unless fm_full."""
    o = opts or {}
    g = math.gcd(I, D)
    i, d = I // g, D // g
    if o.get("fm_poly", 0) >= 0 and not o.get("fm_full") and i == 1 and 2 <= d <= 8 and -(-L // d) <= 768:
        return "poly"
    if L > 4095:
        return "per channel"
    lg, best = None, 0.0
    for c, (a, b) in ((10, (200.0, 0.10)), (11, (300.0, 0.17)), (12, (800.0, 0.16))):
        if (1 << c) < L + 1:
            continue
        sc = float((1 << c) - L + 1)
        v = (a + b * sc) / sc
        if lg is None or v < best:
            lg, best = c, v
    f = o.get("fft_log2f", 0)
    if 10 <= f <= 12 and (1 << f) >= L + 1:
        lg = f
    if -(-d // i) >= (1 << lg) - L + 1:
        return "per channel"
    if lg == 11 and i == 1 and d >= 2 and d % 2 == 0 and ((2048 - L + 1) - d - 1) // 2 > 0 and not o.get("fm_full"):
        return "half"
    return "full"


def proto_taps(L):
    """a Hamming-windowed low-pass of L taps, unit gain in its passband"""
    k = np.arange(L, dtype=np.float64)
    return (0.04 * np.sinc(0.04 * (k - (L - 1) / 2)) * np.hamming(L)).astype(np.complex64) if L > 3 else \
        np.array([0.5 + 0.1j, 0.3 - 0.2j, 0.2 + 0.05j][:L], np.complex64)


def case_taps(L, nchan):
    """chan_taps with a gain of its own on every channel: no two channels alike, down to one tap"""
    gain = np.array([(1 + 0.25 * c) * np.exp(0.7j * c) for c in range(nchan)])
    return (chan_taps(proto_taps(L), nchan).astype(np.complex128) * gain[:, None]).astype(np.complex64)


def chan_sig(n, seed, nchan):
    """sig() plus a tone near every channel's centre: every channel has a signal of its own to get wrong"""
    t = np.arange(n, dtype=np.float64)
    x = sig(n, seed).astype(np.complex128)
    for c in range(nchan):
        x += 0.25 * np.exp(2j * np.pi * (c / max(nchan, 1) - 0.5 + 0.0007) * t + 1j * c)
    return x.astype(np.complex64)


def to_rtlsdr_bytes(z):
    """-> (an ODD number of bytes: I/Q pairs and one trailing byte that is never consumed, the samples RtlSdrDecode makes of them)"""
    s = 100.0 / float(np.max(np.abs(np.concatenate([z.real, z.imag]))))
    b = np.empty(2 * len(z) + 1, np.uint8)
    b[0:-1:2] = np.clip(np.round(z.real * s + 127), 0, 255).astype(np.uint8)
    b[1:-1:2] = np.clip(np.round(z.imag * s + 127), 0, 255).astype(np.uint8)
    b[-1] = 200
    return b, run_chain([orc.RtlSdrDecode()], b)


# (name, kernel family the constructor's rules give, taps, I, D, channels, build options, RTL-SDR byte source)
STREAM_CASES = [
    # decimate-first tiles: 768 taps per phase (and one short of it: an odd block, so that A takes both parities)
    ("poly-6144-1:8", "poly", 6144, 1, 8, 3, {}, False),
    ("poly-6143-1:8", "poly", 6143, 1, 8, 3, {}, False),
    ("poly-5376-1:7", "poly", 5376, 1, 7, 3, {}, False),
    ("poly-1536-1:2", "poly", 1536, 1, 2, 3, {}, False),
    ("poly-1535-1:2", "poly", 1535, 1, 2, 4, {}, False),
    ("poly-2-1:2", "poly", 2, 1, 2, 3, {}, False),
    ("poly-1-1:3", "poly", 1, 1, 3, 3, {}, False),
    ("poly-463-3:18", "poly", 463, 3, 18, 3, {}, False),
    ("poly8-463-1:6-9ch", "poly", 463, 1, 6, 9, {"fm_poly": 8}, False),
    ("poly12-463-1:6-9ch", "poly", 463, 1, 6, 9, {"fm_poly": 12}, False),
    ("poly-463-1:8", "poly", 463, 1, 8, 5, {}, False),
    # just past the decimate-first limits
    ("past-6145-1:8", "per channel", 6145, 1, 8, 3, {}, False),
    ("past-1537-1:2", "full", 1537, 1, 2, 3, {}, False),
    ("past-463-1:9", "full", 463, 1, 9, 3, {}, False),
    # shared-forward tiles, full-size inverse
    ("full-700-1:1", "full", 700, 1, 1, 3, {}, False),
    ("full-701-1:1", "full", 701, 1, 1, 3, {}, False),
    ("full-300-3:2", "full", 300, 3, 2, 3, {}, False),
    ("full-299-3:2", "full", 299, 3, 2, 3, {}, False),
    ("full-200-5:1", "full", 200, 5, 1, 3, {}, False),
    ("full-400-2:3", "full", 400, 2, 3, 3, {}, False),
    ("full-399-2:3", "full", 399, 2, 3, 4, {}, False),
    ("full-2467-25:128", "full", 2467, 25, 128, 3, {}, False),
    ("full-3330-1:9", "full", 3330, 1, 9, 3, {}, False),
    ("full-4000-1:9", "full", 4000, 1, 9, 3, {}, False),
    ("full-4087-1:9", "full", 4087, 1, 9, 3, {}, False),
    ("full-4088-1:9", "per channel", 4088, 1, 9, 3, {}, False),
    ("full-463-1:6-forced", "full", 463, 1, 6, 3, {"fm_full": 1}, False),
    # half-size inverse
    ("half-463-1:6", "half", 463, 1, 6, 3, {"fm_poly": -1}, False),
    ("half-463-1:50", "half", 463, 1, 50, 3, {}, False),
    ("half-600-1:200", "half", 600, 1, 200, 3, {}, False),
    ("half-601-1:200", "half", 601, 1, 200, 4, {}, False),
    ("half-463-1:1582-top", "half", 463, 1, 1582, 3, {}, False),              # ((2048 - 463 + 1) - 1582 - 1) / 2 = 1
    ("half-1991-1:54-top", "half", 1991, 1, 54, 3, {"fft_log2f": 11}, False),   # 58 samples a tile: ((58) - 54 - 1) / 2 = 1
    # RTL-SDR bytes: an odd byte address, an odd byte count
    ("u8-poly-463-1:6", "poly", 463, 1, 6, 3, {}, True),
    ("u8-full-463-1:9", "full", 463, 1, 9, 3, {}, True),
    ("u8-half-463-1:50", "half", 463, 1, 50, 3, {}, True),
]


def stream_plan(L, I, D):
    """-> (S, cap_in, cap_out, n): an input window of more than three filter blocks, an output window for an ODD number of
    them, about 0.6 of the input's — so the output window ends most calls (WAIT_DST) and a.A = n1 moves by an odd multiple
    of S — both windows ODD, cap_out at least one block's ceil(S I / D); a dozen calls or more"""
    S = nsamples(L)
    cap_in = max(int(3.3 * S), 15_000) | 1
    k = max(1, int(0.6 * cap_in / S))
    k -= 1 - (k & 1)
    cap_out = max(_n2(S, I, D), k * S * I // D + 1) | 1
    return S, cap_in, cap_out, min(400_000, 8 * cap_in)


def model_bytes(S, I, D, calls):
    """model() for the RTL-SDR byte source: windows, `consumed` and the WAIT_SRC `need` count bytes"""
    return [(st, 2 * c, p, 2 * need if st == WAIT_SRC else need) for st, c, p, need in model(S, I, D, [(n // 2, cap) for n, cap in calls])]


def series_model(taps0, I, D, src, calls):
    """The protocol of the per-channel composition, Series::work_dev (csrc/compose.cpp) restated over the oracle's blocks:
    inside one work() the blocks take turns, joined by streams of the reference's capacity, until a round moves nothing;
    WAIT_DST is the last block's, WAIT_SRC asks for what the starved block lacks."""
    u8 = np.asarray(src).dtype == np.uint8
    blocks = ([orc.RtlSdrDecode()] if u8 else []) + [orc.FftFilter(taps0), orc.RationalResampler(I, D)]
    m = len(blocks)
    cap = max(4_096_000 // 8, 2 * nsamples(len(taps0)))
    links = [np.zeros(0, b.out_dtype) for b in blocks[:-1]]
    pos, out = 0, []
    for in_len, out_cap in calls:
        win = src[pos:pos + in_len]
        consumed = produced = 0
        last, lneed = [AGAIN] * m, [0] * m
        while True:
            progress = False
            for i, b in enumerate(blocks):
                inp = win[consumed:] if i == 0 else links[i - 1]
                room = out_cap - produced if i == m - 1 else cap - len(links[i])
                st, c, p, nd, o = b.work(inp, room)
                last[i], lneed[i] = st, nd
                if i == 0:
                    consumed += c
                elif c:
                    links[i - 1] = links[i - 1][c:]
                if i == m - 1:
                    produced += p
                else:
                    links[i] = np.concatenate([links[i], o])
                progress = progress or bool(c or p)
            if not progress:
                break
        if last[-1] == WAIT_DST:
            out.append((WAIT_DST, consumed, produced, lneed[-1]))
        elif last[0] == WAIT_SRC:
            nd = lneed[0]
            for j in range(1, m):
                if last[j] != WAIT_SRC or lneed[j] <= len(links[j - 1]):
                    continue
                want, ok = lneed[j] - len(links[j - 1]), True
                for i in range(j - 1, -1, -1):
                    if blocks[i].name == "RtlSdrDecode":
                        want *= 2
                    elif i > 0 or blocks[i].name != "FftFilter":
                        ok = False
                        break
                if ok:
                    nd = max(nd, want)
                break
            out.append((WAIT_SRC, consumed, produced, nd))
        else:
            assert consumed or produced
            out.append((AGAIN, consumed, produced, 0))
        pos += consumed
    return out


def expected_log(family, taps0, I, D, src, calls):
    S = nsamples(len(taps0))
    if family == "per channel":
        return series_model(taps0, I, D, src, calls)
    return model_bytes(S, I, D, calls) if np.asarray(src).dtype == np.uint8 else model(S, I, D, calls)


def ring_calls(expect, n_src, cap_in, cap_out):
    """the calls drive() makes — a ring refilled to cap_in before every work() — with `expect(calls)` the block's answers;
    -> (calls, log)"""
    calls, log, pos, have = [], [], 0, 0
    for _ in range(1_000_000):
        take = min(cap_in - have, n_src - pos)
        have += take; pos += take
        calls.append((have, cap_out))
        log = expect(calls)
        st, c, p, need = log[-1]
        have -= c
        if take == 0 and c == 0 and p == 0:
            return calls, log
    raise AssertionError("no termination")


def launches(log, S, u8=False):
    """a.A = n1 of every call that ran the kernel (at least one whole filter block emitted): the block's n1 is the whole
    blocks within the samples consumed so far"""
    tot, n1, A = 0, 0, []
    for st, c, p, need in log:
        tot += c // 2 if u8 else c
        if tot // S * S > n1:
            A.append(n1)
        n1 = tot // S * S
    return A


def assert_stream_conditions(name, family, S, I, D, cap_in, cap_out, log, u8):
    assert cap_in & 1 and cap_out & 1 and cap_out >= _n2(S, I, D), (name, cap_in, cap_out)
    assert sum(1 for st, c, p, need in log if p) >= 4, (name, log[:8])
    assert any(st == WAIT_DST for st, *_ in log), (name, log[:8])
    if family != "per channel":
        A = launches(log, S, u8)
        # (A is a multiple of S: an even block — an even tap count — leaves it even for ever)
        assert {a & 1 for a in A} == ({0, 1} if S & 1 else {0}) and sum(1 for a in A if a) >= 3, (name, S, A[:12])


def stream_source(name, n, nchan, u8):
    z = chan_sig(n, sum(name.encode()), nchan)
    return to_rtlsdr_bytes(z) if u8 else (z, z)


def check_three_ways(yg, taps, I, D, src, x, tag):
    """each channel: the oracle's length, 1e-5 of the oracle, and 1e-5 + the oracle's own distance of the float64 statement
    (the triangle inequality: no new number); -> the largest (gpu - oracle, gpu - truth, oracle - truth)"""
    pre = [orc.RtlSdrDecode()] if np.asarray(src).dtype == np.uint8 else []
    worst = [0.0, 0.0, 0.0]
    for ch in range(len(taps)):
        yo = run_chain(pre + [orc.FftFilter(taps[ch]), orc.RationalResampler(I, D)], src)
        assert len(yg[ch]) == len(yo) > 0, (tag, ch, len(yg[ch]), len(yo))
        yt = resampled_filter_truth(taps[ch], x, I, D, len(yo))
        e_go, e_gt, e_ot = max_norm_err(yg[ch], yo), max_norm_err(yg[ch], yt), max_norm_err(yo, yt)
        print(f"{tag} ch{ch}: n={len(yo)} gpu-oracle {e_go:.3g} gpu-truth {e_gt:.3g} oracle-truth {e_ot:.3g}")
        assert e_go <= TOL, (tag, ch, e_go, int(np.argmax(np.abs(yg[ch] - yo))))
        assert e_gt <= TOL + e_ot, (tag, ch, e_gt, e_ot, int(np.argmax(np.abs(yg[ch] - yt))))
        worst = [max(a, b) for a, b in zip(worst, (e_go, e_gt, e_ot))]
    return worst


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_streaming_edges_equal_oracle_and_truth(rr, case):
    """Every kernel family at its edges, driven in small ODD windows: a dozen emitting calls with a.A != 0 of both parities
    (where the filter block is odd), WAIT_DST in between, channel windows an odd number of elements apart — odd channels sit at
    8-byte-only addresses — and distinct taps per channel.  Each channel equals its oracle chain in length and within 1e-5,
    and the float64 statement of the operation within 1e-5 plus the oracle's own distance from it; the protocol log is the
    model's."""
    name, family, L, I, D, nchan, opts, u8 = case
    assert expected_kernel(L, I, D, opts) == family
    taps = case_taps(L, nchan)
    assert nchan >= 3 and len({t.tobytes() for t in taps}) == nchan
    S, cap_in, cap_out, n = stream_plan(L, I, D)
    assert S == orc.fftfilter_dims(orc.FftFilter(taps[0]))[1]
    src, x = stream_source(name, n, nchan, u8)
    with rr.build_options(**opts):
        blk = (rr.ChannelizerU8 if u8 else rr.Channelizer)(taps, I, D)
    assert ("per channel" in blk.name) == (family == "per channel"), blk.name       # fused, or the composition
    cin = (2 * cap_in) | 1 if u8 else cap_in
    calls = []
    yg, log = drive(blk, src, nchan, cin, cap_out, offset=1 if u8 else 0, calls=calls)
    assert_stream_conditions(name, family, S, I, D, cin, cap_out, log, u8)
    assert log == expected_log(family, taps[0], I, D, src, calls), name
    check_three_ways(yg, taps, I, D, src, x, name)


# ---- caller-owned windows ------------------------------------------------------------------------------------------------
_OWNED = {"poly": (463, 1, 6, {}), "full": (463, 1, 9, {}), "half": (463, 1, 50, {})}


@pytest.mark.parametrize("u8", [False, True], ids=["c32", "u8"])
@pytest.mark.parametrize("kind", ["poly", "full", "half"])
def test_registered_windows(rr, kind, u8):
    """five channels on PAGE-LOCKED rings (harness.drive_registered: the kernels store into host memory in place, the read
    window moves by what was consumed, the write window starts at a different odd offset on every call, the channel windows
    lie an odd number of elements apart): the oracle's samples within 1e-5, the log of the same block on pageable windows"""
    L, I, D, opts = _OWNED[kind]
    assert expected_kernel(L, I, D, opts) == kind
    taps = case_taps(L, 5)
    S, cap_in, cap_out, n = stream_plan(L, I, D)
    src, x = stream_source(kind, n, 5, u8)
    cin = (2 * cap_in) | 1 if u8 else cap_in
    mk = lambda: (rr.ChannelizerU8 if u8 else rr.Channelizer)(taps, I, D)
    with rr.build_options(**opts):
        ya, la = drive_pageable(mk(), src, cin, cap_out)
        yb, lb = drive_registered(rr, mk(), src, cin, cap_out)
    assert la == lb and sum(1 for st, c, p, need in lb if p) >= 4 and any(st == WAIT_DST for st, *_ in lb)
    assert ya.shape == yb.shape
    check_three_ways(yb, taps, I, D, src, x, f"registered-{kind}")
    check_three_ways(ya, taps, I, D, src, x, f"pageable-{kind}")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("nchan", [2, 9])
@pytest.mark.parametrize("kind", ["poly", "full", "half"])
def test_device_windows_multi(rr, kind, nchan, off):
    """rr_block_work_dev on DEVICE windows (torch tensors only provide the memory): nchan windows an odd out_cap apart,
    starting at element 0 or 1 of the allocation, over several calls — bit-equal to the same block on host windows, same
    log, and not one element outside [c out_cap, c out_cap + produced) touched (sentinels before every call)"""
    import torch
    L, I, D, opts = _OWNED[kind]
    taps = case_taps(L, nchan)
    S, cap_in, cap_out, _ = stream_plan(L, I, D)
    x = chan_sig(6 * cap_in, 40 + nchan, nchan)
    with rr.build_options(**opts):
        host, hlog = drive(rr.Channelizer(taps, I, D), x, nchan, cap_in, cap_out)
        blk = rr.Channelizer(taps, I, D)
    dx = torch.from_numpy(x.view(np.float32).copy()).cuda()
    total = off + nchan * cap_out + 5
    sentinel = np.full(total, np.complex64(complex(-7777.25, 3333.5)), np.complex64)
    dy = torch.from_numpy(sentinel.view(np.float32).copy()).cuda()
    fill = dy.clone()
    got, log, pos, fed = [[] for _ in range(nchan)], [], 0, 0
    for _ in range(10_000):
        in_len = min(cap_in, len(x) - pos)              # drive()'s ring: refilled to cap_in before every call
        take, fed = pos + in_len - fed, pos + in_len
        dy.copy_(fill)
        torch.cuda.synchronize()
        st, c, p, need = blk.work_dev(dx.data_ptr() + 8 * pos, in_len, dy.data_ptr() + 8 * off, cap_out)
        blk.sync()
        y = dy.cpu().numpy().view(np.complex64)
        log.append((st, c, p, need))
        untouched = np.ones(total, bool)
        for ch in range(nchan):
            lo = off + ch * cap_out
            got[ch].append(y[lo:lo + p].copy())
            untouched[lo:lo + p] = False
        assert np.array_equal(y[untouched].view(np.uint64), sentinel[untouched].view(np.uint64)), (kind, nchan, off, len(log), p,
                                                                                                    np.flatnonzero(untouched & (y.view(np.uint64) != sentinel.view(np.uint64)))[:8])
        pos += c
        if take == 0 and c == 0 and p == 0:
            break
    else:
        raise AssertionError("no termination")
    assert log == hlog and sum(1 for st, c, p, need in log if p) >= 4
    for ch in range(nchan):
        yd = np.concatenate(got[ch])
        assert len(yd) == len(host[ch]) > 1000 and np.array_equal(yd.view(np.uint64), host[ch].view(np.uint64)), (kind, nchan, off, ch)


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
