"""Test-side statements about the N-station FM receiver (rr_fm_receiver_create): the window protocol as a Python model,
the test signals (one station for all channels, or one per channel) and the conditions they must meet, the oracle chain of six blocks, the float64 truth of the whole chain and
the propagated parity bar.  Nothing here touches the GPU library; tests/test_fm_receiver_cpu.py checks these statements
against the oracle, tests/test_gpu_fm_receiver.py holds the block to them."""
from __future__ import annotations

from math import gcd

import numpy as np

from harness import WAIT_DST, WAIT_SRC, run_chain
from oracle import pyoracle as orc

ATAN2_EXACT, ATAN2_FAST, DEMOD_FASTFM = 0, 1, 2
TOL = 1e-5


def nsamples(ntaps: int) -> int:
    """the reference's FftFilter block length for a tap count (fft_filter.rs:261-262), asked of the oracle"""
    return orc.fftfilter_dims(orc.FftFilter(np.ones(ntaps, np.complex64)))[1]


class ReceiverModel:
    """The work() protocol of include/rustradio_amd.h rr_fm_receiver_create, from lengths alone.
    A(k) = ceil(floor(d(k S1) / S2) S2 I2 / D2), d(y) = max(N2(y) - 1, 0) for QuadratureDemod, N2(y) for FastFM,
    N2(y) = ceil(y I1 / D1)."""

    def __init__(self, rf_ntaps, rf_interp, rf_deci, audio_ntaps, audio_interp, audio_deci, fastfm=False, u8=False):
        g1, g2 = gcd(rf_interp, rf_deci), gcd(audio_interp, audio_deci)
        self.I1, self.D1, self.I2, self.D2 = rf_interp // g1, rf_deci // g1, audio_interp // g2, audio_deci // g2
        self.S1, self.S2 = nsamples(rf_ntaps), nsamples(audio_ntaps)
        self.fastfm, self.u8 = fastfm, u8
        self.K, self.pend = 0, 0

    def d(self, y):
        r = -(-y * self.I1 // self.D1)
        return r if self.fastfm else max(r - 1, 0)

    def A(self, k):
        return -(-(self.d(k * self.S1) // self.S2 * self.S2) * self.I2 // self.D2)

    def work(self, in_len, out_cap):
        """-> (status, consumed, produced, need) of one call; advances the model"""
        n = in_len // 2 if self.u8 else in_len
        K, S1 = self.K, self.S1
        a0 = self.A(K)
        if self.A(K + 1) - a0 > out_cap:
            return (WAIT_DST, 0, 0, self.A(K + 1) - a0)
        k_in = (self.pend + n) // S1
        k_out = 1
        while self.A(K + k_out + 1) - a0 <= out_cap and k_out <= k_in:
            k_out += 1
        if k_in > k_out:
            k, c, self.pend = k_out, k_out * S1 - self.pend, 0
            st, need = WAIT_DST, self.A(K + k + 1) - self.A(K + k)
        else:
            k, c = k_in, n
            self.pend = self.pend + n - k * S1
            st, need = WAIT_SRC, S1 - self.pend
        self.K += k
        if self.u8:
            c *= 2
            need = need * 2 if st == WAIT_SRC else need
        return (st, c, self.A(K + k) - a0, need)


# ---- signals: one FM station in every channel's passband ---------------------------------------------------------------
def fm_band(fs, n, station_hz, dev_hz, tone_hz, seed, noise=1e-3):
    """a band of FM stations (deviation dev_hz, tones tone_hz + 37 i Hz) at station_hz[i], equal amplitudes summing to 1,
    plus complex noise of sigma `noise`"""
    t = np.arange(n, dtype=np.float64)
    r = np.random.default_rng(seed)
    x = noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for i, f in enumerate(station_hz):
        phi = 2 * np.pi * np.cumsum(f + dev_hz * np.sin(2 * np.pi * (tone_hz + 37.0 * i) * t / fs)) / fs
        x += np.exp(1j * phi) / len(station_hz)
    return x.astype(np.complex64)


def shifted(proto, fs, centres_hz):
    """the prototype low-pass shifted to each channel centre -> [nchan][ntaps] complex64"""
    k = np.arange(len(proto), dtype=np.float64)
    return np.stack([(np.asarray(proto).astype(np.complex128) * np.exp(2j * np.pi * f * k / fs)).astype(np.complex64) for f in centres_hz])


def sinc_low_pass(ntaps, cutoff):
    """an n-tap Hamming low-pass (cutoff in cycles per sample) with unit DC gain, for tap counts a designer would not give"""
    if ntaps == 1:
        return np.array([0.75], np.float32)
    k = np.arange(ntaps) - (ntaps - 1) / 2.0
    h = 2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(ntaps)
    return (h / h.sum()).astype(np.float32)


def to_rtlsdr_bytes(z):
    """Complex samples -> RTL-SDR bytes at half scale (decoded: (b - 127) * 0.008, rtlsdr_decode.rs:35-42)"""
    b = np.empty(2 * len(z), np.uint8)
    b[0::2] = np.clip(np.round(z.real / 0.008 * 0.5 + 127), 0, 255).astype(np.uint8)
    b[1::2] = np.clip(np.round(z.imag / 0.008 * 0.5 + 127), 0, 255).astype(np.uint8)
    return b


class Shape:
    """one receiver shape with its signal: taps [C][L1], ratios, audio taps, scale, and the band the stations live in"""

    def __init__(self, name, taps, rf, audio_taps, audio, scale, x, skip, gain=1.0, mode=ATAN2_EXACT):
        self.name, self.taps, self.rf, self.audio_taps, self.audio = name, np.asarray(taps, np.complex64), rf, np.asarray(audio_taps, np.float32), audio
        self.scale, self.x, self.skip, self.gain, self.mode = scale, x, skip, gain, mode    # skip: demodulated samples of RF start-up

    @property
    def nchan(self):
        return len(self.taps)

    def model(self, u8=False):
        return ReceiverModel(self.taps.shape[1], *self.rf, len(self.audio_taps), *self.audio, fastfm=self.mode == DEMOD_FASTFM, u8=u8)


def shape_cfg4(n=300_000, nchan=32, seed=5):
    """configs[3]-like: the configs[2] low-pass (2.4 Msps, 100 kHz, 463 taps) shifted by multi.cfg4_taps, 1:6, audio 3:25.
    The bank's own 8 kHz raster spreads 32 channels over 248 kHz, more than one 200 kHz passband: no single station lies in all
    of them, and 32 stations of their own would each be heard by a dozen neighbours.  So the 32 channels sit on a 1.5 kHz
    raster (cfg4_taps' spacing argument) around ONE station at +100 kHz with 50 kHz deviation: every passband holds all of it.
    The shifted taps select a band without translating it, so every channel demodulates 2 pi (100 kHz +- 50 kHz) / 400 kHz:
    at most 0.75 pi, and large enough that the plain term of the bar is not dwarfed by the propagated one."""
    from rustradio_amd import multi
    proto = orc.low_pass_complex(multi.CFG4_FS, 100e3, 12.5e3)
    c0 = 128 + 67 - nchan // 2
    taps = multi.cfg4_taps(proto, range(c0, c0 + nchan), spacing_hz=1.5e3)
    x = fm_band(multi.CFG4_FS, n, [100e3], 50e3, 1e3, seed)
    return Shape("cfg4", taps, (1, 6), orc.low_pass(400e3, 20e3, 4e3), (3, 25), 0.5, x, 463 // 6 + 2)


def shape_rtl_fm(n=500_000, seed=6):
    """examples/rtl_fm.rs:381-419 at its own rates: 1.024 Msps, low_pass_complex(1.024e6, 100e3, 1000) = 2467 taps shifted to
    four channel centres, 25:128 to 200 kHz, low_pass(200e3, 44.1e3, 500), 6:25.  The shifted taps select a band without
    translating it and the 25:128 resampler picks samples 5 or 6 apart, so a carrier away from 0 turns by a different angle
    from pick to pick (-400 kHz: 0.09 pi and -0.69 pi): the four centres lie +-5 and +-15 kHz around ONE station at 0 with
    50 kHz deviation (2 pi 50 kHz 6 / 1.024 MHz = 0.59 pi at most), inside every passband."""
    fs, centres = 1.024e6, [-15e3, -5e3, 5e3, 15e3]
    proto = orc.low_pass_complex(fs, 100e3, 1000.0)
    assert len(proto) == 2467
    x = fm_band(fs, n, [0.0], 50e3, 1e3, seed)
    return Shape("rtl_fm", shifted(proto, fs, centres), (25, 128), orc.low_pass(200e3, 44.1e3, 500.0), (6, 25), 0.25, x,
                 2467 * 25 // 128 + 2)


def shape_small(rf_deci, audio_ntaps, audio, n=None, seed=7, nchan=3, mode=ATAN2_EXACT, rf_interp=1):
    """three channels with distinct taps around one station, RF decimation 5 or 50 (and any other), audio filters of any tap
    count.  fs = 1 MHz; the channel rate is fs I / D, the station's excursion stays below 0.3 of it and inside the passband"""
    fs = 1e6
    rate = fs * rf_interp / rf_deci
    proto = orc.low_pass_complex(fs, 0.35 * rate, 0.15 * rate)
    centres = [0.05 * rate * (c - (nchan - 1) / 2) for c in range(nchan)]
    n = n or int(max(60_000, 8000 * rf_deci / rf_interp))
    x = fm_band(fs, n, [0.0], 0.22 * rate, 0.01 * rate, seed)
    return Shape(f"small-{rf_interp}:{rf_deci}-{audio_ntaps}-{audio[0]}:{audio[1]}", shifted(proto, fs, centres), (rf_interp, rf_deci),
                 sinc_low_pass(audio_ntaps, 0.2 * min(1.0, audio[0] / audio[1])), audio, -1.5, x,
                 len(proto) * rf_interp // rf_deci + 2, mode=mode)


# ---- signals: one FM station OF ITS OWN per channel ---------------------------------------------------------------------
def fm_stations(fs, n, station_hz, dev_hz, tone_hz, seed, noise=1e-3):
    """station i at station_hz[i] with its own deviation dev_hz[i] and tone tone_hz[i], amplitudes 1 / len(station_hz), plus
    complex noise of sigma `noise`"""
    t = np.arange(n, dtype=np.float64)
    r = np.random.default_rng(seed)
    x = noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for f, dev, tone in zip(station_hz, dev_hz, tone_hz):
        phi = 2 * np.pi * np.cumsum(f + dev * np.sin(2 * np.pi * tone * t / fs)) / fs
        x += np.exp(1j * phi) / len(station_hz)
    return x.astype(np.complex64)


def shape_distinct(nchan, rf_deci, audio_ntaps=65, audio=(2, 3), fs=1e6, n=None, seed=11, transition=0.15, mode=ATAN2_EXACT, live=None):
    """nchan channels, each with a station no other channel hears.  Integer decimation, rf_interp = 1: the channel rate is
    fs / rf_deci.  The shifted taps select a band without translating it, so only centres at integer multiples of the channel
    rate fold to DC behind the resampler: channel i sits at (i - nchan // 2) x rate (nchan <= rf_deci of them are distinct),
    and station i sits on centre i with deviation (0.17 + 0.01 (i % 8)) rate and tone (0.004 + 0.0031 (i % 11)) rate — the
    audio of two channels differs by thousands of bars (test_fm_receiver_cpu.py asserts at least 100 for every pair), so a
    receiver that hands a channel any other channel's carry, history, row or verdict fails parity.  Smaller deviations
    (0.10 - 0.22 rate) leave the bar of a channel with a small start-up spike above 10 x plain nearly everywhere.
    The propagated term of the bar over the plain one is about 5 sum|audio_taps| / (peak angle), and sum|h| of a windowed sinc
    grows with ntaps x cutoff (128 taps at 0.2: 2.1, 900 at 0.13: 2.8 — every sample above 10 x plain), so long audio filters
    get the cutoff 8 / ntaps (sum|h| about 1.7) and the tones are slowed until the fastest lies at half the cutoff.
    The stream holds 60 audio filter lengths per channel at least: the start-up stretch, where |r| is small and the bar wide,
    stays below 2 % of the samples.  `transition` (of the rate) sets the prototype's tap count.  `live`: every channel's RF
    taps but that one are zero (the silent-channel tests)."""
    assert 1 <= nchan <= rf_deci, (nchan, rf_deci)
    rate = fs / rf_deci
    proto = orc.low_pass_complex(fs, 0.35 * rate, transition * rate)
    centres = [(i - nchan // 2) * rate for i in range(nchan)]
    n = n or int(rf_deci * max(8000, 60 * audio_ntaps))
    cutoff = min(0.2 * min(1.0, audio[0] / audio[1]), 8.0 / audio_ntaps)
    slow = min(1.0, cutoff / 0.07)
    x = fm_stations(fs, n, centres, [(0.17 + 0.01 * (i % 8)) * rate for i in range(nchan)],
                    [(0.004 + 0.0031 * (i % 11)) * slow * rate for i in range(nchan)], seed)
    taps = shifted(proto, fs, centres)
    if live is not None:
        taps[[c for c in range(nchan) if c != live]] = 0
    return Shape(f"distinct-{nchan}x1:{rf_deci}-{audio_ntaps}-{audio[0]}:{audio[1]}" + ("" if live is None else f"-live{live}"), taps,
                 (1, rf_deci), sinc_low_pass(audio_ntaps, cutoff), audio, -1.5, x, len(proto) // rf_deci + 2, mode=mode)


# the distinct-station signals of tests/test_gpu_fm_receiver.py by name: (channels, RF decimation, audio taps, audio ratio, keywords).
# tests/test_fm_receiver_cpu.py holds every one of them to the signal conditions and to the separation of its channels.
DISTINCT = {
    "4x10": (4, 10, 65, (2, 3), {}),
    "9x10": (9, 10, 65, (2, 3), {}),
    "9x10-u8": (9, 10, 65, (2, 3), {}),
    "5x5": (5, 5, 128, (7, 4), {}),
    "32x40": (32, 40, 65, (2, 3), {}),
    "5x6-2.4M": (5, 6, 241, (3, 25), dict(fs=2.4e6)),                          # 97 RF taps: the decimate-first tiles at 1:6
    "5x6-2.4M-463": (5, 6, 241, (3, 25), dict(fs=2.4e6, transition=0.03125)),   # 463 RF taps, cfg4's count: every FmMulti family
    "5x10-400": (5, 10, 400, (2, 3), {}),                                      # audio tile 2048 by cost, 1024 beside it
    "9x10-400": (9, 10, 400, (2, 3), {}),
    "9x10-900": (9, 10, 900, (2, 3), {}),                                      # audio tile 4096 by cost, 2048 beside it
    "5x5-65": (5, 5, 65, (2, 3), {}),
    "5x5-u8": (5, 5, 128, (7, 4), {}),
    "9x10-400-u8": (9, 10, 400, (2, 3), {}),
}
STREAM_KINDS = ("mixed", "short-in", "tight-out")


def distinct(key, **kw):
    nchan, deci, ant, audio, k = DISTINCT[key]
    return shape_distinct(nchan, deci, ant, audio, **dict(k, **kw))


def fuzz_distinct(seed):
    """the second fuzz family: a distinct-station shape, a source type and four windows drawn from the seed
    -> (shape, u8, [(input window, output window)])"""
    g = np.random.default_rng(7000 + seed)
    nchan = int(g.choice([2, 3, 5, 9, 17]))
    deci = int(g.choice([d for d in (2, 3, 5, 6, 8, 10, 25) if d >= nchan]))
    ant = int(g.choice([1, 2, 17, 64, 65, 200, 511]))
    audio = [(2, 3), (7, 4), (1, 1), (3, 25), (6, 25), (1, 4), (4, 2)][int(g.integers(0, 7))]
    u8 = bool(g.integers(0, 2))
    n = int(g.integers(50_000, 90_000))
    n = max(n, 6 * nsamples(ant) * deci)                              # six audio blocks at least
    sh = shape_distinct(nchan, deci, ant, audio, seed=100 + seed, n=n)
    m = sh.model(u8)
    S1 = m.S1 * (2 if u8 else 1)
    step = max(max(m.A(k + 1) - m.A(k) for k in range(n // m.S1 + 1)), 1)
    caps = [(int(g.integers(S1 // 3 + 1, 6 * S1)), int(g.integers(max(step // 2, 1), 5 * step + 2))) for _ in range(3)] + [(4 * S1 + 1, 3 * step + 1)]
    return sh, u8, caps


def stream_caps(m: ReceiverModel, kind, n):
    """the windows of the streaming tests, (input, output) per call in turn: input windows shorter than one RF block, output
    windows below the next step (WAIT_DST consuming nothing) and between steps (WAIT_DST after k_out blocks)"""
    S1 = m.S1 * (2 if m.u8 else 1)
    step = max(m.A(k + 1) - m.A(k) for k in range(n // m.S1 + 1))
    if kind == "mixed":
        return [(3 * S1 + 7, 2 * step + 3), (S1 // 2 + 1, step - 1), (5 * S1 + 1, step), (S1 + 3, 6 * step + 1)]
    if kind == "short-in":
        return [(S1 // 3 + 1, 4 * step + 5), (S1 // 2 + 2, 4 * step + 5), (2 * S1 + 1, 4 * step + 5)]
    assert kind == "tight-out", kind
    return [(9 * S1 + 5, step), (9 * S1 + 5, step // 2), (9 * S1 + 5, 2 * step + 1)]


class ModelBlock:
    """the protocol model behind a block's work(): zeros for samples.  Lets a CPU test drive the GPU tests' own loop"""

    def __init__(self, m: ReceiverModel, nchan):
        self.m, self.nchan = m, nchan

    def work(self, x, out_cap):
        st, c, p, need = self.m.work(len(x), out_cap)
        return st, c, p, need, np.zeros((self.nchan, p), np.float32)


def drive(blk, x, nch, caps):
    """Graph::run's loop around the block with per-call window capacities caps[i % len] = (input, output) -> ([nch] streams, log)"""
    outs, log = [[] for _ in range(nch)], []
    pos, ring, idle = 0, np.zeros(0, x.dtype), 0
    for i in range(200_000):
        cin, cout = caps[i % len(caps)]
        take = max(0, min(cin - len(ring), len(x) - pos))
        ring = np.concatenate([ring, x[pos:pos + take]]); pos += take
        st, c, p, need, out = blk.work(ring[:cin], cout)
        log.append((len(ring[:cin]), cout, st, c, p, need))
        ring = ring[c:]
        out = np.atleast_2d(out)
        for ch in range(nch):
            outs[ch].append(out[ch])
        idle = idle + 1 if (take == 0 and c == 0 and p == 0) else 0
        if idle >= len(caps):
            break
    else:
        raise AssertionError("no termination")
    return [np.concatenate(o) for o in outs], log


def call_lengths(m: ReceiverModel, log):
    """what the model says every call of `log` ((input window, output window, ...) per call) took in: -> [(RF blocks, new
    demodulated samples, filtered audio samples n_y, audio samples produced)] — n_y = 0 with new demodulated samples is the
    call that only carries (k_audio_multi_carry)"""
    out = []
    for cin, cout, *_ in log:
        K0 = m.K
        st, c, p, need = m.work(cin, cout)
        d0, d1 = m.d(K0 * m.S1), m.d(m.K * m.S1)
        out.append((m.K - K0, d1 - d0, (d1 // m.S2 - d0 // m.S2) * m.S2, p))
    return out


def neighbour_distance(sh: Shape, chans=None, x=None):
    """|au_c - au_c'| / bar_c over the samples behind the start-up tenth, for every ordered pair of `chans` (all by default)
    -> {(c, c'): (median, max, share of samples within the bar)}; the oracle alone"""
    chans = list(range(sh.nchan) if chans is None else chans)
    au, bar = {}, {}
    for c in chans:
        au[c], _dm, r = oracle_channel(sh, c, x)
        bar[c], _ = audio_bar(sh, r, au[c])
    out = {}
    for c in chans:
        for d in chans:
            if c != d:
                lo = len(au[c]) // 10
                q = np.abs(au[c][lo:].astype(np.float64) - au[d][lo:]) / bar[c][lo:]
                out[(c, d)] = (float(np.median(q)), float(np.max(q)), float(np.mean(q <= 1.0)))
    return out


# ---- the reference chain, its float64 truth and the parity bar ---------------------------------------------------------
def demodulator(gain, mode):
    return orc.FastFM() if mode == DEMOD_FASTFM else orc.QuadratureDemod(gain, mode)


def oracle_channel(sh: Shape, ch: int, x=None, stream_bytes=4_096_000):
    """-> (audio, demodulated, resampled) streams of channel ch through the six oracle blocks (examples/rtl_fm.rs:381-419),
    stage by stage: every block's whole-stream output depends on its whole-stream input only"""
    x = sh.x if x is None else x
    r = run_chain([orc.FftFilter(sh.taps[ch]), orc.RationalResampler(*sh.rf)], x, stream_bytes=stream_bytes)
    dm = run_chain([demodulator(sh.gain, sh.mode)], r, stream_bytes=stream_bytes)
    au = run_chain([orc.FftFilterFloat(sh.audio_taps), orc.RationalResampler(*sh.audio, dtype=np.float32), orc.MultiplyConst(sh.scale)],
                   dm, stream_bytes=stream_bytes)
    return au, dm, r


def signal_conditions(dm, r, skip):
    """after the RF start-up: max |angle| <= 0.9 pi and min |r| >= 0.1 max |r| — no +-pi wrap flip reaches the linear audio filter"""
    ang = float(np.max(np.abs(dm[skip:])))
    mag = np.abs(r[skip:].astype(np.complex128))
    return ang, float(mag.min() / mag.max())


def audio_bar(sh: Shape, r, ref, tol=TOL):
    """bar[m] = |scale| (|audio_taps| * b)[q] + tol max|ref|, q = (m D2) // I2 the filtered sample audio sample m is, b the
    per-sample bound of harness.angle_parity on the oracle's resampled stream r -> (bar, plain term)"""
    mag = np.abs(np.asarray(r).astype(np.complex128))
    eps = tol * float(mag.max())
    b = abs(sh.gain) * (tol * np.pi + eps / np.maximum(mag[:-1], 1e-30) + eps / np.maximum(mag[1:], 1e-30))
    prop = np.convolve(np.abs(sh.audio_taps.astype(np.float64)), b)[:len(b)]
    g = gcd(*sh.audio)
    q = (np.arange(len(ref), dtype=np.int64) * (sh.audio[1] // g)) // (sh.audio[0] // g)
    plain = tol * float(np.max(np.abs(ref)))
    return abs(sh.scale) * prop[q] + plain, plain


def float64_truth(sh: Shape, ch: int, n_out: int, x=None):
    """the whole chain in float64, no block, ring or tile: complex128 convolution, out[r] = y[(r D) // I], the angle of
    r[m + 1] conj(r[m]), a real convolution, the second index map, the scale (QuadratureDemod only)"""
    x = (sh.x if x is None else x).astype(np.complex128)
    t = sh.taps[ch].astype(np.complex128)
    m = 1 << int(np.ceil(np.log2(len(x) + len(t))))
    y = np.fft.ifft(np.fft.fft(x, m) * np.fft.fft(t, m))[:len(x)]
    g1, g2 = gcd(*sh.rf), gcd(*sh.audio)
    I1, D1, I2, D2 = sh.rf[0] // g1, sh.rf[1] // g1, sh.audio[0] // g2, sh.audio[1] // g2
    nr = -(-len(y) * I1 // D1)
    r = y[(np.arange(nr, dtype=np.int64) * D1) // I1]
    dm = sh.gain * np.angle(r[1:] * np.conj(r[:-1]))
    a = sh.audio_taps.astype(np.float64)
    m2 = 1 << int(np.ceil(np.log2(len(dm) + len(a))))
    f = np.fft.irfft(np.fft.rfft(dm, m2) * np.fft.rfft(a, m2), m2)[:len(dm)]
    q = (np.arange(n_out, dtype=np.int64) * D2) // I2
    assert n_out == 0 or q[-1] < len(f)
    return sh.scale * f[q]
