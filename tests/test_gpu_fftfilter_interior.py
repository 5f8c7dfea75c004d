"""FftFilter's tile kernel walks each workgroup's tiles in three parts: edge tiles (the window touches the carried prefix or
the start of the stream, or the tile reaches past n_out) through the staging routine and the per-element store, and the run
of interior tiles between them in a loop of its own, instantiated per `row0 = first / T` (first = ntaps - 1, T = F / 16),
that advances a load and a store pointer and asks no tile anything (csrc/kernels_fft.hip InteriorIO / interior_run).  These
tests put the seams of that split under calls through work_dev on device windows: every output of every call against the
oracle (TOL, the bar of test_gpu_parity), the work() protocol against the oracle's, and bit for bit against the edge-tile
path where the same tile can be made to take it.

Free arguments, fixed here: the stream is uniform noise in [-1, 1) (seeded), the taps are noise / (L // 4); a call's window
is `in_len` samples from the first unconsumed one and its output window `out_cap` samples.  On the flagship shape (401
taps, forced 2048-point tile) a reference block is NS = 623 samples and a tile advances S = 1648."""
import numpy as np
import pytest

from harness import knob, max_norm_err
from oracle import pyoracle as orc
from test_gpu_parity import TOL, both, rnd_c

pytestmark = pytest.mark.gpu

NS, S, BIG = 623, 1648, 1 << 40


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


def taps_for(L):
    return rnd_c(L, 300 + L) / max(1, L // 4)


def drive(blk, x, calls, dev):
    """[(in_len, out_cap), ...] -> ([(status, consumed, produced, need), ...], [out of each call]); `dev`: through work_dev
    on device windows (x lives on the device once, a call's window is a pointer into it), else work() on host windows."""
    pos, log, outs = 0, [], []
    if dev:
        import torch
        dx = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    for in_len, out_cap in calls:
        if pos >= len(x):
            break
        in_len = min(in_len, len(x) - pos)
        out_cap = min(out_cap, in_len + NS_MAX)
        if dev:
            dy = torch.zeros(2 * max(out_cap, 1), dtype=torch.float32, device="cuda")
            st, c, p, need = blk.work_dev(dx.data_ptr() + 8 * pos, in_len, dy.data_ptr(), out_cap)
            blk.sync()
            out = dy.cpu().numpy().view(np.complex64)[:p].copy()
        else:
            st, c, p, need, out = blk.work(x[pos:pos + in_len], out_cap)
        log.append((st, c, p, need))
        outs.append(out)
        pos += c
    return log, outs


NS_MAX = 1 << 14      # (more than any pending count: an output window "as large as it can matter")


def check(rr, taps, x, calls):
    """the calls on a fresh block of each side: same protocol, every output within TOL of the oracle's -> the GPU's outputs"""
    lo, yo = drive(orc.FftFilter(taps), x, calls, False)
    lg, yg = drive(rr.FftFilter(taps), x, calls, True)
    assert lg == lo, "work() protocol differs from the reference restatement"
    ref, got = np.concatenate(yo), np.concatenate(yg)
    assert len(got) == len(ref) and len(ref) > 0
    e = max_norm_err(got, ref)
    assert e <= TOL, e
    return yg


def flagship(rr, monkeypatch, **opts):
    knob(rr, monkeypatch, fft_log2f=11, **opts)
    taps = taps_for(401)
    assert rr.fftfilter_dims(rr.FftFilter(taps)) == (1024, NS, 2048)
    return taps


# n_out -> tiles: 623 -> 1 (edge), 1869 -> 2 (both edge), 3738 -> 3 (edge, ONE interior, edge), 13706 -> 9.  Nine tiles are a
# grid of nine workgroups (grid = min(tiles, CUs x resident workgroups per CU), and no part this runs on has fewer than nine
# CUs) over TileIter's eight partitions [9 x / 8, 9 (x + 1) / 8): partitions 0 .. 6 hold one tile, partition 7 holds tiles 7
# and 8.  Workgroups 0 .. 6 take ONE tile each, workgroup 7 takes TWO (tile 7 interior, then tile 8, the edge tile), and
# workgroup 8, the second of partition 0, starts at tile 1 >= its partition's end: NO tile.
@pytest.mark.parametrize("name,calls", [
    ("one_reference_block", [(NS, BIG)]),
    ("two_tiles_no_interior", [(3 * NS, BIG)]),
    ("one_interior_tile", [(6 * NS, BIG)]),
    ("nine_tiles_a_workgroup_without_one", [(22 * NS, BIG)]),
    ("later_calls_pending_0", [(6 * NS, BIG), (22 * NS, BIG), (NS, BIG), (6 * NS, BIG)]),
    ("later_calls_pending_622", [(6 * NS + 622, BIG), (22 * NS, BIG), (1, BIG), (3 * NS - 1, BIG), (6 * NS, BIG)]),
    ("output_window_ends_the_call", [(30 * NS + 100, 6 * NS), (30 * NS + 100, 7 * NS + 300), (30 * NS, BIG)]),
])
@pytest.mark.parametrize("tail", [0, 3])
def test_tile_counts_and_carried_state(rr, monkeypatch, name, calls, tail):
    """First call on zero history (tile 0 reads the prefix), later calls behind 0 and behind NS - 1 pending samples; `tail`
    3 runs the same through the kernel that carries the non-finite pass in its tail (another instance of the split)."""
    taps = flagship(rr, monkeypatch, **({"fft_nonfinite_tiles": 3} if tail else {}))
    x = rnd_c(sum(c[0] for c in calls) + 5, len(calls) + 17 * len(name))
    yg = check(rr, taps, x, calls)
    if name == "one_reference_block":
        assert [len(y) for y in yg] == [NS]
    if name == "later_calls_pending_622":
        assert len(yg[2]) == NS, "the one-sample call completes the pending block"


@pytest.mark.parametrize("L,blocks,rest", [(409, 16, 0),        # 16 x 615 = 9840 = 6 tiles of 1640: ends on a tile
                                           (465, 17, -1),       # 17 x 559 = 9503 = 6 tiles of 1584 - 1: one output short
                                           (472, 20, 1)])       # 20 x 552 = 11040 = 7 tiles of 1577 + 1: one output past
def test_last_tile_ends_at_n_out(rr, monkeypatch, L, blocks, rest):
    """The last tile inside n_out to its last position is interior; one output short of that it is an edge tile."""
    knob(rr, monkeypatch, fft_log2f=11)
    taps = taps_for(L)
    _, ns = orc.fftfilter_dims(orc.FftFilter(taps))
    n_out = blocks * ns
    assert (n_out - rest) % (2048 - L + 1) == 0
    x = rnd_c(n_out + 5, 7 * L + blocks)
    yg = check(rr, taps, x, [(n_out + 5, BIG)])
    assert len(yg[0]) == n_out, "one call with exactly this many outputs is the case under test"


def row_cases():
    out = []
    for log2f in (10, 11, 12):
        T = 1 << (log2f - 4)
        # row0 = 0 (first % T = 0 and T - 1), 1 (both), 3 (both; 2048 points also the flagship's first = 400), and the
        # largest the tile admits, 15 (first % T = 0 and T - 2: a forced tile takes at most F - 1 taps)
        firsts = [0, T - 1, T, 2 * T - 1, 3 * T, 4 * T - 1, 15 * T, 16 * T - 2] + ([400] if log2f == 11 else [])
        out += [(log2f, f) for f in firsts]
    return out


@pytest.mark.parametrize("log2f,first", row_cases())
def test_rows_on_every_tile_size(rr, monkeypatch, log2f, first):
    """One call of seven tiles and a part (at least two reference blocks), then the same stream in calls of two and a half
    tiles: with first >= S several tiles of a call start inside the carried prefix before the interior run begins."""
    knob(rr, monkeypatch, fft_log2f=log2f)
    F, L = 1 << log2f, first + 1
    St = F - first
    taps = taps_for(L)
    ref_fft, ns, tile = rr.fftfilter_dims(rr.FftFilter(taps))
    assert tile == F, "the forced tile was not taken"
    n = max(7 * St + St // 3, 2 * ns) + first
    x = rnd_c(n, L + log2f)
    one = check(rr, taps, x, [(n, BIG)])
    chunk = max(2 * St + St // 2, ns + 1)
    many = check(rr, taps, x, [(chunk, BIG)] * (n // chunk + 3))
    assert len(np.concatenate(many)) == len(one[0])


@pytest.fixture(scope="module")
def large():
    """10 000 reference blocks of the flagship shape in one call: 3781 tiles (3781 % 8 = 5), three or four per resident
    workgroup -> (taps, x, oracle output); computed once, read by the tests below"""
    taps = taps_for(401)
    x = rnd_c(10_000 * NS + 77, 6230)
    lo, yo = drive(orc.FftFilter(taps), x, [(len(x), BIG)], False)
    assert lo[0][2] == 10_000 * NS and -(-lo[0][2] // S) == 3781
    return taps, x, yo[0]


@pytest.mark.parametrize("tail", [0, 3])
def test_more_interior_tiles_than_workgroups(rr, monkeypatch, large, tail):
    """Every workgroup advances its pointers over several interior tiles; every one of the 6.23e6 outputs is compared."""
    knob(rr, monkeypatch, fft_log2f=11, **({"fft_nonfinite_tiles": 3} if tail else {}))
    taps, x, yo = large
    lg, yg = drive(rr.FftFilter(taps), x, [(len(x), BIG)], True)
    assert lg[0][2] == len(yo)
    e = max_norm_err(yg[0], yo)
    assert e <= TOL, e


def test_interior_tiles_equal_the_edge_path_bit_for_bit(rr, monkeypatch, large):
    """The same window with a shorter output window: the tile that holds the last outputs now reaches past n_out and takes
    the edge path (same loads, the per-element store) where the long call had it in the interior loop.  Its outputs, and
    all before them, are the same bits.  Cuts at 6 .. 40 reference blocks: the last tile is tile 2 .. 15, cut at 25 different
    places of a tile."""
    knob(rr, monkeypatch, fft_log2f=11)
    taps, x, _ = large
    w = x[:60 * NS]
    _, ya = drive(rr.FftFilter(taps), w, [(len(w), BIG)], True)
    assert len(ya[0]) == 60 * NS
    for k in range(6, 41):
        lg, yb = drive(rr.FftFilter(taps), w, [(len(w), k * NS)], True)
        assert lg[0][2] == k * NS
        assert np.array_equal(yb[0].view(np.uint32), ya[0][:k * NS].view(np.uint32)), k


def test_firfilter_on_the_same_tiles(rr, monkeypatch):
    """FirFilter on overlap-save tiles runs a third instance of the kernel (its non-finite repair in the tail)."""
    knob(rr, monkeypatch, fir_path="fft", fir_prune=-1, fir_half=-1, fir_poly=-1)
    taps = taps_for(401)
    assert rr.fir_uses_fft_tiles(rr.FirFilter(taps))
    x = rnd_c(40_000, 4010)
    both(rr, lambda m: [m.FirFilter(taps)], x, stream_bytes=8 * (len(x) + 16))
    both(rr, lambda m: [m.FirFilter(taps)], x, stream_bytes=8 * 5000)
