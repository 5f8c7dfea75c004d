"""The tile transforms after the constant rotations of Dft<8> / Dft<16> moved into the butterflies' FMAs (csrc/fft_core.hpp):
rr.FftFilter against a float64 np.convolve of the same taps, within TOL of the output's max, on every tile size and with
inputs that single out the registers and the outputs of the butterflies.

Tile sizes (the block's own choice, asserted): 33 taps -> 1024 points (16 * 16 * 4), 401 -> 2048 (16 * 16 * 8), 1025 -> 4096
(16 * 16 * 16), 2467 -> 8192 as two 4096-point sub-transforms (k_fftfilt_split).  The block takes the split tile by itself only
for windows of some 4.6 M samples (FftFilter::alt_wins; below that it runs the same taps on plain 4096-point tiles), which
no float64 convolution of 2467 taps follows in a test's time: that case forces the tile size, which leaves the split kernel
as the only one the block has, and asserts that it ran.

Windows hold three tiles and a part of a fourth, and every case runs two of them through one block, so that the second
call starts in the carried prefix.  Inputs:
  - one unit impulse in each of the 16 register rows of the first call's second tile (tile position n T + (7 n + 3) % T,
    T = F / 16: pass 0 loads v[n] = tile[n T + t]), real and imaginary — the reference is np.convolve of that one sample
    with the taps, put at its place (every other product of the full convolution is an exact zero);
  - one complex tone on a bin of the tile's transform per output digit d of the last forward pass (bin 53 + 256 d: the last
    pass's digit is the most significant one; on the split tile the bin of the sub-transform, 2 (53 + 256 d) + d % 2);
  - seeded noise.
One FirFilter (127 taps, on overlap-save tiles) and one fused FM chain case against the oracle, since they share the
butterflies.

Worst error / output max as measured on MI355X (TOL is 1e-5): impulses 1.0e-7 / 1.6e-7 / 1.8e-7 / 2.3e-7 on the 1024- / 2048- /
4096- / 8192-point tiles, tones and noise 4.6e-7 / 4.4e-7 / 4.7e-7 / 6.0e-7, FirFilter 3.6e-7."""
import numpy as np
import pytest

from harness import knob, max_norm_err, run_chain
from oracle import pyoracle as orc
from test_gpu_parity import TOL, _demod_close, both, fm_signal, rnd_c

pytestmark = pytest.mark.gpu

SIZES = [(33, 10, None), (401, 11, None), (1025, 12, None), (2467, 13, "split")]
LAST_RADIX = {10: 4, 11: 8, 12: 16, 13: 16}


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


def taps_for(L):
    return rnd_c(L, 900 + L) / max(1, L // 4)


def setup(rr, monkeypatch, L, log2f, kernel):
    if kernel == "split":
        knob(rr, monkeypatch, fft_log2f=log2f)
    taps = taps_for(L)
    F = 1 << log2f
    assert rr.fftfilter_dims(rr.FftFilter(taps))[2] == F
    S = F - L + 1
    return taps, F, S, 3 * S + S // 3 + L


def run_two_windows(rr, taps, x, W, kernel):
    """x through one block in windows of W samples -> (output, calls that emitted)"""
    b, lg = rr.FftFilter(taps), []
    y = run_chain([b], x, stream_bytes=8 * W, log=lg)
    if kernel:
        assert b.last_kernel() == kernel
    return y, sum(1 for r in lg if r[3] > 0)


def check(y, ref, calls, what, worst):
    assert calls >= 2 and len(ref) - len(y) < 8192, (what, calls, len(y), len(ref))
    e = max_norm_err(y, ref[:len(y)].astype(np.complex64))
    worst[0] = max(worst[0], e)
    assert e <= TOL, (what, e)


@pytest.mark.parametrize("L,log2f,kernel", SIZES, ids=[f"F{1 << s[1]}" for s in SIZES])
def test_impulse_in_every_register_row(rr, monkeypatch, L, log2f, kernel):
    taps, F, S, W = setup(rr, monkeypatch, L, log2f, kernel)
    T, t128, worst = F // 16, taps.astype(np.complex128), [0.0]
    for n in range(16):
        at = S + n * T + (7 * n + 3) % T - (L - 1)                   # tile 1 of the first call, row n
        assert 0 <= at < W - L
        for val in (1.0, 1.0j):
            x = np.zeros(2 * W, np.complex64)
            x[at] = val
            ref = np.zeros(2 * W, np.complex128)
            ref[at:at + L] = np.convolve(x[at:at + 1].astype(np.complex128), t128)
            y, calls = run_two_windows(rr, taps, x, W, kernel)
            check(y, ref, calls, (n, val), worst)
    print(f"F={F}: worst impulse error / max {worst[0]:.3e}")


@pytest.mark.parametrize("L,log2f,kernel", SIZES, ids=[f"F{1 << s[1]}" for s in SIZES])
def test_tone_per_output_digit_and_noise(rr, monkeypatch, L, log2f, kernel):
    taps, F, S, W = setup(rr, monkeypatch, L, log2f, kernel)
    t128, worst = taps.astype(np.complex128), [0.0]
    n = np.arange(2 * W, dtype=np.float64)
    for d in range(LAST_RADIX[log2f]):
        k = 2 * (53 + 256 * d) + d % 2 if kernel == "split" else 53 + 256 * d
        assert k < F
        x = np.exp(2j * np.pi * ((k * n) % F) / F).astype(np.complex64)
        y, calls = run_two_windows(rr, taps, x, W, kernel)
        check(y, np.convolve(x.astype(np.complex128), t128)[:2 * W], calls, ("tone", d), worst)
    print(f"F={F}: worst tone error / max {worst[0]:.3e}")
    x = rnd_c(2 * W, 77 + L)
    y, calls = run_two_windows(rr, taps, x, W, kernel)
    check(y, np.convolve(x.astype(np.complex128), t128)[:2 * W], calls, "noise", worst)
    print(f"F={F}: worst tone / noise error / max {worst[0]:.3e}")


def test_fir_filter_on_tiles_and_fm_chain(rr, monkeypatch):
    knob(rr, monkeypatch, fir_path="fft")
    taps = taps_for(127)
    assert rr.fir_uses_fft_tiles(rr.FirFilter(taps))
    x = rnd_c(8000, 127)
    e = both(rr, lambda m: [m.FirFilter(taps)], x, stream_bytes=8 * 4000)
    print(f"FirFilter 127 taps: error / max {e:.3e}")
    lp = orc.low_pass_complex(1.024e6, 100e3, 6.4e3)
    z = fm_signal(40_000, 1.024e6, 0.0, 127)
    yo = run_chain([orc.FftFilter(lp), orc.RationalResampler(1, 5), orc.QuadratureDemod(1.0)], z)
    ro = run_chain([orc.FftFilter(lp), orc.RationalResampler(1, 5)], z)
    d = _demod_close(run_chain([rr.FmChain(lp, 1, 5, 1.0)], z), yo, ro)
    print(f"FmChain 1:5: worst angle error {float(np.max(d)) / np.pi:.3e} pi")
