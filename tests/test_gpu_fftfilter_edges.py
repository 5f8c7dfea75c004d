"""FftFilter's tile loads and stores at the edges of their addressing: every kind of position of `first = L - 1` inside a
row of T = F / 16 tile positions (first % T = 0, 1, T - 1, mid-row; first < T: row 0 straddles and nothing is skipped), on
each tile size, and windows that end on, one past and one short of a tile, that are shorter than a tile, that arrive in
small calls (tiles that start inside the carried prefix, the first fast tile behind a slow one) and that hold more tiles
than there are resident workgroups.  The tile kernel addresses a tile as scalar base + lane offset + immediate and decides
which rows it stores from `first` alone (csrc/kernels_fft.hip load_tile16 / TileStore); the decimating FirFilter and the
fused FM chain share the loads.  Reference: the oracle, as in test_gpu_parity.test_fftfilter; same bar (TOL)."""
import numpy as np
import pytest

from harness import knob, run_chain
from oracle import pyoracle as orc
from test_gpu_parity import TOL, _demod_close, both, fm_signal, rnd_c

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


def taps_for(L):
    return rnd_c(L, 300 + L) / max(1, L // 4)


@pytest.mark.parametrize("log2f,L", [(10, 2), (10, 17), (10, 64), (10, 65), (10, 66), (10, 128), (10, 129),
                                     (11, 257), (11, 384), (11, 385), (11, 386), (11, 401), (11, 512), (11, 513),
                                     (12, 1025), (12, 1500), (12, 2049)])
def test_first_on_every_row_position(rr, monkeypatch, log2f, L):
    """Six tiles and a part of a seventh in one call, then the same stream in calls of about two tiles (the second call's
    first tile starts inside the carried prefix)."""
    knob(rr, monkeypatch, fft_log2f=log2f)
    F = 1 << log2f
    S = F - L + 1
    taps = taps_for(L)
    assert rr.fftfilter_dims(rr.FftFilter(taps))[2] == F, "the forced tile was not taken"
    x = rnd_c(6 * S + S // 3 + L, L + log2f)
    both(rr, lambda m: [m.FftFilter(taps)], x, stream_bytes=8 * (len(x) + 16))
    both(rr, lambda m: [m.FftFilter(taps)], x, stream_bytes=8 * (2 * S + L + 100))


@pytest.mark.parametrize("L,blocks,rest", [(409, 16, 0),        # 16 x 615 = 9840 = 6 tiles of 1640: ends on a tile
                                           (472, 20, 1),        # 20 x 552 = 11040 = 7 tiles of 1577 + 1: one output past
                                           (465, 17, -1),       # 17 x 559 = 9503 = 6 tiles of 1584 - 1: one output short
                                           (401, 2, None)])     # 2 x 623 = 1246 < 1648: shorter than a tile
def test_window_ends_around_a_tile(rr, monkeypatch, L, blocks, rest):
    knob(rr, monkeypatch, fft_log2f=11)
    S = 2048 - L + 1
    taps = taps_for(L)
    _, ns = orc.fftfilter_dims(orc.FftFilter(taps))
    n_out = blocks * ns
    if rest is None:
        assert n_out < S
    else:
        assert (n_out - rest) % S == 0 and n_out > 3 * S
    x = rnd_c(n_out + 5, 7 * L + blocks)
    lg = []
    yg = run_chain([rr.FftFilter(taps)], x, stream_bytes=8 * (len(x) + 16), log=lg)
    assert lg[0][3] == n_out, "one call with exactly this many outputs is the case under test"
    assert len(yg) == n_out
    both(rr, lambda m: [m.FftFilter(taps)], x, stream_bytes=8 * (len(x) + 16))


@pytest.mark.parametrize("call", [700, 5000])
def test_stream_in_small_calls(rr, monkeypatch, call):
    """401 taps on 2048-point tiles in calls of 700 samples (one reference block: less than a tile, every tile reads the
    carried prefix) and of 5000 (three tiles and a part: a staged tile, then whole ones)."""
    knob(rr, monkeypatch, fft_log2f=11)
    taps = taps_for(401)
    x = rnd_c(40_000, call)
    both(rr, lambda m: [m.FftFilter(taps)], x, stream_bytes=8 * call)


def test_more_tiles_than_workgroups(rr, monkeypatch):
    """One window of 2.5e6 samples: 1517 tiles of 1648 outputs (1517 % 8 = 5), more than the 1024 workgroups a launch keeps
    resident — workgroups go on to a second tile, and the eight partitions of the tile range meet at uneven seams."""
    knob(rr, monkeypatch, fft_log2f=11)
    taps = taps_for(401)
    n = 2_500_000
    n_out = n // 623 * 623
    assert -(-n_out // 1648) == 1517
    x = rnd_c(n, 2500)
    both(rr, lambda m: [m.FftFilter(taps)], x, stream_bytes=8 * (n + 16))


def test_shared_tile_loads_decimating_fir_and_fm_chain(rr, monkeypatch):
    """The same 401 taps through the two other kernels on these tile loads: a decimating FirFilter on overlap-save tiles
    and the fused FftFilter -> RationalResampler -> QuadratureDemod chain."""
    taps = taps_for(401)
    knob(rr, monkeypatch, fir_path="fft", fir_prune=-1, fir_half=-1, fir_poly=-1, fm_poly=-1)
    x = rnd_c(60_000, 401)
    assert rr.fir_uses_fft_tiles(rr.FirFilter(taps, deci=4))
    both(rr, lambda m: [m.FirFilter(taps, deci=4)], x)
    both(rr, lambda m: [m.FirFilter(taps, deci=4)], x[:25_000], stream_bytes=8 * 5000)
    lp = orc.low_pass_complex(1.024e6, 100e3, 6.4e3)
    z = fm_signal(80_000, 1.024e6, 0.0, 401)
    for I, D in ((25, 128), (1, 5)):
        yo = run_chain([orc.FftFilter(lp), orc.RationalResampler(I, D), orc.QuadratureDemod(1.0)], z)
        ro = run_chain([orc.FftFilter(lp), orc.RationalResampler(I, D)], z)
        _demod_close(run_chain([rr.FmChain(lp, I, D, 1.0)], z), yo, ro)
