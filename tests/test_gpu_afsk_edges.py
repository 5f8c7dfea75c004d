"""GPU: the kernel edges of rr.AfskDemod, taken from rr_afsk_demod_dims — first pushes of 1 / 2 / 0 samples, a stream fed one sample
at a time past the carry, pushes around a tile, a push shorter than the carry between two long ones, 4,096 streams, strides above n
with a sentinel beyond every count, and a NaN sample at a tile's first and last sample and inside the carry.  Everything is held
bit for bit to the same stream in one push."""
import numpy as np
import pytest

import afsk_dev as ad
import afsk_model as am
import rustradio_amd as rr
from symsync_dev import u32

pytestmark = pytest.mark.gpu
H, L = 9, 21                                  # a short carry (30 samples): the one-sample pushes stay few


def handle(ns=1, h=H, l=L):
    return rr.AfskDemod(ns, h, am.lp_taps(l), 1.0, -0.125)


@pytest.fixture(scope="module")
def dims():
    tile, carry = handle().dims()
    assert carry == H + L
    return tile, carry


@pytest.fixture(scope="module")
def long_row(dims):
    """2 tiles + 3 samples of two streams and their outputs in one push (shared, read-only)"""
    tile, _ = dims
    x = np.stack([am.two_tone(2 * tile + 3, c) for c in range(2)])
    whole = ad.dev_push(handle(2), x)
    x.setflags(write=False)
    whole.setflags(write=False)
    return x, whole


def test_first_pushes_of_one_two_and_no_samples(long_row):
    x, whole = long_row
    h = handle(2)
    a = ad.dev_push(h, x[:, :1])
    assert a.shape == (2, 0)                                  # one sample in all: no output yet
    b = ad.dev_push(h, x[:, 1:3])
    assert b.shape == (2, 2)
    c = ad.dev_push(h, x[:, 3:3])
    assert c.shape == (2, 0)
    d = ad.dev_push(h, x[:, 3:])
    assert ad.same_bits(np.concatenate([a, b, c, d], axis=1), whole)


def test_one_sample_at_a_time_past_the_carry(dims, long_row):
    """carry + 2 pushes of one sample: every one splices the old carry and one new sample"""
    _, carry = dims
    x, whole = long_row
    k = carry + 2
    got = ad.run_pushes(handle(2), x[:, :k + 40], [1] * k + [40])
    assert ad.same_bits(got, whole[:, :k + 39])


@pytest.mark.parametrize("first", [-1, 0, 1])
def test_pushes_around_a_tile(dims, long_row, first):
    """tile - 1, tile, tile + 1 samples as the first push (tile - 2 .. tile outputs) and again as the second"""
    tile, _ = dims
    x, whole = long_row
    n = x.shape[1]
    a = tile + first
    for lens in ([a, n - a], [5, a, n - a - 5]):
        assert ad.same_bits(ad.run_pushes(handle(2), x, lens), whole), lens


def test_a_push_shorter_than_the_carry_between_two_long_ones(dims, long_row):
    tile, carry = dims
    x, whole = long_row
    n = x.shape[1]
    for short in (1, 2, carry - 1, carry):
        lens = [tile + 7, short, n - tile - 7 - short]
        assert ad.same_bits(ad.run_pushes(handle(2), x, lens), whole), lens


def test_a_halo_longer_than_a_tile_in_short_pushes(dims):
    """L = tile + 1: every push below the carry, the halo of a tile reaching through several pushes"""
    tile, _ = dims
    n = 2 * tile + 3
    x = am.two_tone(n, 5)
    whole = ad.dev_push(handle(1, 65, tile + 1), x)
    lens = [700] * (n // 700) + [n % 700]
    assert ad.same_bits(ad.run_pushes(handle(1, 65, tile + 1), x, lens), whole)


def test_four_thousand_streams():
    """4,096 x 70 in pushes of 33 and 37: stream c == the same row through a 1-stream handle in one push, for a few c, and all
    rows differ"""
    ns, n = 4096, 70
    i = np.arange(n)
    x = np.stack([(0.3 + 0.0001 * c) * np.cos((0.2 + 0.0001 * c) * i + 0.01 * c) for c in range(ns)]).astype(np.float32)
    got = ad.run_pushes(handle(ns), x, [33, 37])
    assert got.shape == (ns, n - 1)
    for c in (0, 1, 63, 64, 2047, 4095):
        assert ad.same_bits(ad.dev_push(handle(1), x[c]), got[c:c + 1]), c
    assert len({got[c].tobytes() for c in range(ns)}) == ns


def test_strides_above_n_leave_the_gaps_alone(dims, long_row):
    """in_stride n + 5 (the gap holds NaN), out_stride n + 9 (the gap and everything beyond each count holds the sentinel:
    afsk_dev.dev_push asserts it is still there)"""
    tile, _ = dims
    x, whole = long_row
    n = x.shape[1]
    h, parts, at = handle(2), [], 0
    for k in (tile - 3, 1, n - tile + 2):
        parts.append(ad.dev_push(h, x[:, at:at + k], in_stride=k + 5, out_stride=k + 9))
        at += k
    assert ad.same_bits(np.concatenate(parts, axis=1), whole)


@pytest.mark.parametrize("where", ["tile-first", "tile-last", "in-carry"])
def test_a_nan_sample_reaches_exactly_its_own_outputs(dims, where):
    """NaN at x[k]: outputs k .. k + H + L - 1 are NaN, every other output has the bits of the run with x[k] = 0.  k is the sample
    the second tile's first output sits on, the one its last sits on, and one that the second push finds in the carry."""
    tile, carry = dims
    n = 2 * tile + 3 + H + L
    k = {"tile-first": tile, "tile-last": 2 * tile - 1, "in-carry": tile - 5}[where]
    lens = [n] if where != "in-carry" else [tile, n - tile]
    x = am.two_tone(n, 9)
    x0, xn = x.copy(), x.copy()
    x0[k], xn[k] = 0.0, np.nan
    clean = ad.run_pushes(handle(), x0, lens)[0]
    got = ad.run_pushes(handle(), xn, lens)[0]
    hit = np.zeros(n - 1, bool)
    hit[k:k + H + L] = True
    assert hit.sum() == H + L
    assert np.all(np.isnan(got[hit])) and np.all(np.isfinite(clean))
    assert np.array_equal(u32(got[~hit]), u32(clean[~hit]))
