"""GPU: the blocks that pick their kernel PER work() CALL, by the size of the window, switched in mid-stream under the
default selection (no rr_build_opts: a forced path turns the per-call choice off).

FmChain / FmChainU8 / FirFmChain take the decimate-first tiles ("poly"), the half-size inverse ("half"), the plain 4096-point
tile of a long filter ("alt"), its split 8192-point tile ("split") or the plain tile ("full"); FftFilter and the fused
FirFilter -> FftFilter with 2100..3584 composite taps take "alt" or "split"; HilbertFir takes the pruned real-stream tile
("prune", which writes the carried history itself) or the direct form ("direct", history by a carry launch).  The crossovers
lie at 1.2 M ... 6 M samples on 256 CUs, above every ring the other streaming tests use, so here one stream alternates
between windows on either side of them and the state one family hands to the next is what is checked: the prefix
[history | pending], the carried r, the non-finite verdict slots (whose probe stride is the CURRENT call's), the head fix of
the fused FirFilter -> FftFilter blocks (first emitting call, whatever its family) and HilbertFir's history.

The thresholds are restated from csrc/blocks.cpp and the device's CU count; every window lies at least MARGIN = 1.3x on its
side of each crossover (one exception, stated at the 1:2 case), and rr_debug_last_kernel must report, call by call, the
families the schedule was built for: a rule that moves makes the case FAIL instead of passing without a switch.

Per case: the (status, consumed, produced, need) log is the oracle chain's seen at the fused block's boundary, the lengths
are equal, the samples are within the suite's bars (filters: max_norm_err <= TOL; chains: the propagated angle bound).  The
NaN cases ask for the oracle's NaN set exactly."""
import numpy as np
import pytest

from harness import AGAIN, angle_parity, max_norm_err
from oracle import pyoracle as orc
from test_gpu_parity import TOL, fm_signal, rnd_c, rnd_f

pytestmark = pytest.mark.gpu

MARGIN = 1.3
AMPLE = 1 << 17          # output room beyond the window's length: more than one reference block of any filter here


@pytest.fixture(scope="module")
def rr():
    import rustradio_amd
    return rustradio_amd


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- the driver ---------------------------------------------------------------------------------------------------------
class Run:
    """y: the last block's output; log: per call, the (status, consumed, produced, need) of every block; fams: the family
    rr_debug_last_kernel reports after each emitting call (library blocks); mid: the output of block `keep`; takes: the new
    samples every call's window got"""

    def __init__(self):
        self.y, self.log, self.fams, self.mid, self.takes = None, [], [], None, []


def drive_schedule(blocks, x, caps=None, takes=None, keep=None):
    """harness.run_chain's loop with a per-call list of input-window sizes `caps` (cycled) and an ample output window: call k
    sees what the last call left unconsumed (as in harness.Ring) plus new samples up to caps[k] in all; every block of the
    chain runs once per call on everything the block before it has produced.  One call per window: the stream ends with the
    call that took the last samples.  takes = [...] replays the new samples per call of another run instead (a chain whose
    first block holds nothing back sees the same windows further down that way)."""
    x = np.asarray(x, blocks[0].in_dtype)
    left = [np.zeros(0, b.in_dtype) for b in blocks]
    r, pos, outs, mids = Run(), 0, [], []
    for k in range(64):
        if takes is not None:
            if k >= len(takes):
                break
            take = takes[k]
        else:
            if pos >= len(x):
                break
            take = min(max(caps[k % len(caps)] - len(left[0]), 0), len(x) - pos)
        win = np.concatenate([left[0], x[pos:pos + take]])
        pos += take
        r.takes.append(take)
        call = []
        for i, b in enumerate(blocks):
            st, c, p, need, out = b.work(win, len(win) + AMPLE)
            call.append((st, c, p, need))
            left[i] = win[c:].copy()
            if keep == i:
                mids.append(out)
            if i + 1 < len(blocks):
                win = np.concatenate([left[i + 1], out])
        r.log.append(tuple(call))
        outs.append(out)
        if hasattr(blocks[-1], "last_kernel") and call[-1][2]:
            r.fams.append(blocks[-1].last_kernel())
    else:
        raise AssertionError("drive_schedule: more than 64 calls")
    assert pos == len(x), (pos, len(x))
    r.y = np.concatenate(outs)
    r.mid = np.concatenate(mids) if mids else None
    return r


def fused_view(call, f=0, front=0, unit=1):
    """What ONE block that fuses the oracle's chain reports for the same call: the first block's consumed, the last block's
    produced, and the status and need of the FftFilter at index f (with ample output the only block of these chains that
    waits: WAIT_SRC for the rest of its next block).  need counts the fused block's own window: `unit` elements per sample (2
    for RTL-SDR bytes) plus the `front` samples a front FirFilter holds back in it (fir.rs:537)."""
    st, _, _, need = call[f]
    return (st, call[0][1], call[-1][2], need * unit + front)


def lib_log(run):
    return [c[0] for c in run.log]


def check_families(run, want, tag):
    """the library's own report: exactly the families the windows were built for, every ordered pair of them at least once"""
    print(f"{tag}: families per emitting call: {' '.join(run.fams)}")
    assert run.fams == want, (tag, run.fams, want)
    switches = {(a, b) for a, b in zip(want, want[1:]) if a != b}
    assert len(switches) >= 2, (tag, want)                       # (both directions of at least one switch)
    for pair in switches:
        assert pair in set(zip(run.fams, run.fams[1:])), (tag, pair, run.fams)


# ---- the selection rules (csrc/blocks.cpp), restated -------------------------------------------------------------------
def chip_units(v, cus):
    return max(1, (v * cus + 128) // 256)


def poly_min_inputs(L, D, cus):
    """FmChain, I = 1: decimate-first tiles from chip_units(1000) * (1024 - ceil(L / D)) resampled samples per call on"""
    return chip_units(1000, cus) * (1024 - -(-L // D)) * D


def half_min_inputs(cus):
    """FmChain on 2048-point tiles, even D: the half-size inverse from chip_units(1200000) filtered samples per call on"""
    return chip_units(1_200_000, cus)


def alt_wins(n, L, log2f, chain, cus):
    """FftFilter::alt_wins (csrc/blocks.hpp): the plain 4096-point tile against the split 2^log2f-point tile"""
    cu = cus / 256.0
    na = n / (4096 - L + 1) / cu
    ns = n / ((1 << log2f) - L + 1) / cu
    plain = 13.0 + na * ((0.0112 if na < 2500.0 else 0.0127) if chain else 0.0105)
    split = max(25.0 + 0.022 * ns, 12.0 + 0.032 * (ns + 200.0) if chain else 12.0 + 0.0207 * ns + 2.6e-6 * n / cu)
    return plain < split


def alt_crossover(L, log2f, chain, cus):
    """the one window size below which the plain tile wins and above which the split tile does (checked on a 20,000-sample
    lattice up to 64 M samples)"""
    grid = np.arange(20_000, 64_000_000, 20_000)
    wins = np.array([alt_wins(int(n), L, log2f, chain, cus) for n in grid])
    first = int(np.argmin(wins))
    assert wins[:first].all() and not wins[first:].any() and first > 0, "alt_wins is not a single crossover"
    return int(grid[first])


def prune_min_inputs(Lg, D, cus):
    """HilbertFir, decimation 4 / 8 / 16 on 1024 / 2048 / 4096-point tiles: pruned from chip_units(1500 | 1500 | 350) batches
    of D / 2 tiles of 2 (F - Lg + 1) real samples on"""
    F = {4: 1024, 8: 2048, 16: 4096}[D]
    return chip_units(350 if D == 16 else 1500, cus) * 2 * (F - Lg + 1) * (D // 2)


def below(w, thr, slack):
    """a window of w samples stays MARGIN below a crossover at thr (slack: the pending samples a call may add to it)"""
    assert (w + slack) * MARGIN <= thr, (w, thr)
    return w


def above(w, thr, slack):
    assert w - slack >= MARGIN * thr, (w, thr)
    return w


# ---- inputs, made once -------------------------------------------------------------------------------------------------
_CACHE = {}


def station(n):
    """test_gpu_parity.fm_signal, a centred FM station (|r| stays away from 0): one stream, every chain takes its start"""
    if "fm" not in _CACHE or len(_CACHE["fm"]) < n:
        _CACHE["fm"] = fm_signal(n, 2.4e6, 0.0, 0x5EED0051)
    return _CACHE["fm"][:n]


def noise_c(n):
    if "c" not in _CACHE or len(_CACHE["c"]) < n:
        _CACHE["c"] = rnd_c(n, 0x5EED0052)
    return _CACHE["c"][:n]


def to_bytes(z, odd):
    """what an RTL-SDR delivers for z (test_fm_chain_u8_fused_block), with a trailing odd byte that is never consumed"""
    n = len(z)
    b = np.empty(2 * n + (1 if odd else 0), np.uint8)
    b[0:2 * n:2] = np.clip(np.round(z.real / 0.008 + 127), 0, 255)
    b[1:2 * n:2] = np.clip(np.round(z.imag / 0.008 + 127), 0, 255)
    if odd:
        b[-1] = 200
    return b


TAPS463 = lambda: orc.low_pass_complex(2.4e6, 100e3, 12.5e3)          # noqa: E731  (nsamples 561, 2048-point tiles)
TAPS2467 = lambda: orc.low_pass_complex(1.024e6, 100e3, 1e3)          # noqa: E731  (nsamples 5725, 8192-point split tiles)


def check_chain(run_g, run_o, view, taps_len, D, tag, nan=False):
    """log, length and the chain bar (test_fm_chain_cfg3: the filter stage's 1e-5 propagated through atan2) — with nan=True the
    oracle's NaN set exactly and the bar on the rest (test_nan_sets_of_the_fused_chains_are_the_references)"""
    want = [view(c) for c in run_o.log]
    got = lib_log(run_g)
    assert got == want, (tag, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    yg, yo, ro = run_g.y, run_o.y, run_o.mid
    assert len(yg) == len(yo) > 1000 and len(ro) == len(yo) + 1, (tag, len(yg), len(yo), len(ro))
    skip = taps_len // D + 2
    if nan:
        bo, bg = ~np.isfinite(yo), ~np.isfinite(yg)
        assert 20 < bo.sum() < len(yo), (tag, int(bo.sum()))
        assert np.array_equal(bo, bg), (tag, int(bo.sum()), int(bg.sum()), np.flatnonzero(bo != bg)[:8])
        ro = np.where(np.isfinite(ro.real) & np.isfinite(ro.imag), ro, 1.0)
        yg, yo = np.where(bo, 0.0, yg), np.where(bo, 0.0, yo)
    r = angle_parity(yg, yo, ro, TOL, skip)
    print(f"{tag}: {r['used']:.3f} of the propagated allowance used, largest error {r['max_err_pi']:.2e} pi, {len(yo)} outputs")
    assert r["used"] <= 1.0, (tag, r)
    return r


def check_filter(run_g, run_o, view, tag, nan=False):
    """log, length and max_norm_err <= TOL — with nan=True the oracle's non-finite set exactly and the bar on the rest
    (test_nonfinite_samples_in_fftfilter_poison_the_references_blocks)"""
    want = [view(c) for c in run_o.log]
    got = lib_log(run_g)
    assert got == want, (tag, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    yg, yo = run_g.y, run_o.y
    assert len(yg) == len(yo) > 1000, (tag, len(yg), len(yo))
    ok = np.ones(len(yo), bool)
    if nan:
        bo, bg = ~(np.isfinite(yo.real) & np.isfinite(yo.imag)), ~(np.isfinite(yg.real) & np.isfinite(yg.imag))
        assert 20 < bo.sum() < len(yo), (tag, int(bo.sum()))
        assert np.array_equal(bo, bg), (tag, int(bo.sum()), int(bg.sum()), np.flatnonzero(bo != bg)[:8])
        ok = ~bo
    e = max_norm_err(yg[ok], yo[ok])
    print(f"{tag}: largest error {e:.2e} of the largest sample, {len(yo)} outputs")
    assert e <= TOL, (tag, e)
    return e


# ---- the fused FM chains ----------------------------------------------------------------------------------------------
def fm_windows_1_6(cus):
    """463 taps 1:6: "full" below the half-size inverse's bar, "poly" above the decimate-first tiles'"""
    S = 561
    small = below(half_min_inputs(cus) * 5 // 12, half_min_inputs(cus), S)                   # 0.5 M on 256 CUs
    large = above(int(1.32 * poly_min_inputs(463, 6, cus)), poly_min_inputs(463, 6, cus), S)     # 7.5 M
    return small, large


def test_fm_chain_full_and_poly(rr, cus):
    """FmChain, 463 taps, 1:6: windows of 0.5 M and 7.5 M samples (on 256 CUs) alternate between the plain 2048-point tile and
    the decimate-first tiles; prefix, pending samples and the carried r pass from one to the other in both directions"""
    taps = TAPS463()
    small, large = fm_windows_1_6(cus)
    caps = [small, large, small, large, small]
    x = station(sum(caps))
    g = drive_schedule([rr.FmChain(taps, 1, 6, 0.9)], x, caps)
    check_families(g, ["full", "poly", "full", "poly", "full"], f"FmChain 463 taps 1:6, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps), orc.RationalResampler(1, 6), orc.QuadratureDemod(0.9)], x, caps, keep=1)
    check_chain(g, o, fused_view, len(taps), 6, "FmChain 1:6 full <-> poly")


def test_fm_chain_full_half_and_poly(rr, cus):
    """FmChain, 463 taps, 1:2: three families in one stream, every ordered pair of them once.  The half-size inverse runs
    between 1.2 M filtered samples and the decimate-first bar, 1000 (1024 - 232) 2 = 1.584 M: a band of 1.32x, too narrow for
    a window 1.3x inside both ends.  Its window is the band's geometric middle (1.38 M on 256 CUs, 1.149x from either end;
    the pending samples move a call by less than 561); the other two windows keep the 1.3x."""
    taps = TAPS463()
    S = 561
    h_lo, p_lo = half_min_inputs(cus), poly_min_inputs(463, 2, cus)
    full = below(h_lo * 5 // 12, h_lo, S)
    half = int((h_lo * p_lo) ** 0.5)
    assert (h_lo + S) * 1.14 <= half <= (p_lo - S) / 1.14, (h_lo, half, p_lo)
    poly = above(int(1.32 * p_lo), p_lo, S)
    caps = [full, half, poly, half, full, poly, full]
    x = station(sum(caps))
    g = drive_schedule([rr.FmChain(taps, 1, 2, 0.9)], x, caps)
    check_families(g, ["full", "half", "poly", "half", "full", "poly", "full"], f"FmChain 463 taps 1:2, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps), orc.RationalResampler(1, 2), orc.QuadratureDemod(0.9)], x, caps, keep=1)
    check_chain(g, o, fused_view, len(taps), 2, "FmChain 1:2 full, half, poly")


def test_fm_chain_u8_full_and_poly(rr, cus):
    """FmChainU8, 463 taps, 1:6, RTL-SDR bytes, odd total length: the same switch on the IQ8 loaders.  Windows count bytes (an
    odd number of them for the small ones: a byte stays behind in the window); consumed and need count bytes too."""
    taps = TAPS463()
    small, large = fm_windows_1_6(cus)
    caps = [2 * small + 1, 2 * large, 2 * small + 1, 2 * large, 2 * small + 1]
    b = to_bytes(station((sum(caps) - 3) // 2), odd=True)      # (calls 1 and 3 find a byte in the window: 2 bytes fewer in all)
    g = drive_schedule([rr.FmChainU8(taps, 1, 6, 0.9)], b, caps)
    check_families(g, ["full", "poly", "full", "poly", "full"], f"FmChainU8 463 taps 1:6, {cus} CUs, byte windows {caps}")
    o = drive_schedule([orc.RtlSdrDecode(), orc.FftFilter(taps), orc.RationalResampler(1, 6), orc.QuadratureDemod(0.9)], b, caps, keep=2)
    assert len(b) % 2 == 1 and sum(c[0][1] for c in g.log) == len(b) - 1
    check_chain(g, o, lambda c: fused_view(c, f=1, unit=2), len(taps), 6, "FmChainU8 1:6 full <-> poly")


def test_fm_chain_alt_and_split(rr, cus):
    """FmChain, 2467 taps, 25:128 (the rtl_fm front end): the plain 4096-point chain tile for small windows, the split
    8192-point tile for large ones (FftFilter::alt_wins with the chain's costs; crossover 4.08 M samples on 256 CUs)"""
    taps = TAPS2467()
    assert len(taps) == 2467
    S = 5725
    cross = alt_crossover(2467, 13, True, cus)
    small, large = below(cross // 4, cross, S), above(int(1.32 * cross) + S, cross, S)
    caps = [small, large, small, large, small]
    x = station(sum(caps))
    g = drive_schedule([rr.FmChain(taps, 25, 128, 0.9)], x, caps)
    check_families(g, ["alt", "split", "alt", "split", "alt"], f"FmChain 2467 taps 25:128, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps), orc.RationalResampler(25, 128), orc.QuadratureDemod(0.9)], x, caps, keep=1)
    check_chain(g, o, fused_view, len(taps), 5, "FmChain 25:128 alt <-> split")      # (skip: 2467 / 5 > 2467 * 25 / 128 outputs)


@pytest.mark.parametrize("first", ["small", "large"])
def test_fir_fm_chain_head_fix_then_switches(rr, cus, first):
    """FirFmChain, front 127 + 401 taps (527 composite, 2048-point tiles), 1:4: the head fix runs in the first emitting call,
    under the plain tile (first = small) or under the decimate-first tiles (first = large), and the stream then switches both
    ways.  The front FirFilter holds its last 126 samples back in the window: they ride along in every call."""
    t1, t2 = orc.low_pass_complex(10e6, 1e6, 190e3), orc.low_pass_complex(10e6, 1e6, 60e3)
    assert (len(t1), len(t2)) == (127, 401)
    L, S = 527, 623
    small = below(half_min_inputs(cus) * 5 // 12, half_min_inputs(cus), S)
    large = above(int(1.32 * poly_min_inputs(L, 4, cus)), poly_min_inputs(L, 4, cus), S)
    caps = [small, large, small, large, small] if first == "small" else [large, small, large, small, small]
    fams = ["poly" if c == large else "full" for c in caps]
    x = station(sum(caps) - 126 * (len(caps) - 1))
    g = drive_schedule([rr.FirFmChain(t1, t2, 1, 4, 0.7)], x, caps)
    check_families(g, fams, f"FirFmChain 127 + 401 taps 1:4, {cus} CUs, first call {first}, windows {caps}")
    o = drive_schedule([orc.FirFilter(t1), orc.FftFilter(t2), orc.RationalResampler(1, 4), orc.QuadratureDemod(0.7)], x, caps, keep=2)
    check_chain(g, o, lambda c: fused_view(c, f=1, front=126), len(t2), 4, f"FirFmChain 1:4, first call {first}")


# ---- FftFilter and FirFilter -> FftFilter ------------------------------------------------------------------------------
def filter_windows(rr, blk, L, cus):
    ref_fft, S, tile = rr.fftfilter_dims(blk)
    assert tile == 8192, tile                                   # the split tile, with the plain 4096-point one beside it
    cross = alt_crossover(L, 13, False, cus)
    return S, below(cross // 4, cross, S), above(int(1.32 * cross) + S, cross, S)


def test_fftfilter_alt_and_split(rr, cus):
    """FftFilter, 2467 taps: plain 4096-point tiles below 4.6 M samples per call (256 CUs), split 8192-point tiles above"""
    taps = (rnd_c(2467, 43) / 1000).astype(np.complex64)
    blk = rr.FftFilter(taps)
    S, small, large = filter_windows(rr, blk, 2467, cus)
    caps = [small, large, small, large, small]
    x = noise_c(sum(caps))
    g = drive_schedule([blk], x, caps)
    check_families(g, ["alt", "split", "alt", "split", "alt"], f"FftFilter 2467 taps, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps)], x, caps)
    check_filter(g, o, fused_view, "FftFilter 2467 taps alt <-> split")


@pytest.mark.parametrize("first", ["small", "large"])
def test_fir_fftfilter_head_fix_then_switches(rr, cus, first):
    """FirFftFilter, 127 + 2400 taps (2526 composite): the head fix in a first call on the plain tile or on the split tile,
    then both switches; the first 2399 outputs are also judged against their own scale (test_fir_fftfilter_fused_block)"""
    t1 = orc.low_pass_complex(10e6, 1e6, 190e3)
    t2 = (rnd_c(2400, 2405) / 300).astype(np.complex64)
    blk = rr.FirFftFilter(t1, t2)
    S, small, large = filter_windows(rr, blk, 2526, cus)
    assert S == 8192 - 2400
    caps = [small, large, small, large, small] if first == "small" else [large, small, large, small, small]
    fams = ["split" if c == large else "alt" for c in caps]
    x = noise_c(sum(caps) - 126 * (len(caps) - 1))
    g = drive_schedule([blk], x, caps)
    check_families(g, fams, f"FirFftFilter 127 + 2400 taps, {cus} CUs, first call {first}, windows {caps}")
    o = drive_schedule([orc.FirFilter(t1), orc.FftFilter(t2)], x, caps)
    check_filter(g, o, lambda c: fused_view(c, f=1, front=126), f"FirFftFilter, first call {first}")
    h = len(t2) + 8
    scale = max(float(np.max(np.abs(o.y[:h]))), 1e-3 * float(np.max(np.abs(o.y))))
    assert max_norm_err(g.y[:h], o.y[:h], scale=scale) <= 10 * TOL


# ---- HilbertFir ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("translate", [None, (8.0, 1.0)], ids=["plain", "translate"])
def test_hilbert_fir_prune_and_direct(rr, cus, translate):
    """HilbertFir, Hilbert 31, 64 Complex taps, /4 (94 composite taps on 1024-point real-stream tiles): the pruned tile writes
    the 31 samples of history itself, the direct form leaves them to a carry launch; with .translate() (default rotator) the
    rotator's phase rides through the switches too.  The fused block keeps FirFilter's bookkeeping on the REAL window (its
    last 63 + samples stay in it), the oracle's Hilbert takes all it is given and the FirFilter behind it holds them back: the
    oracle replays the library's new samples per call, and its FirFilter's log is the fused block's."""
    taps = (rnd_c(64, 67) / 8).astype(np.complex64)
    thr = prune_min_inputs(94, 4, cus)
    small, large = below(thr // 5, thr, 8), above(int(1.32 * thr) + 128, thr, 128)
    caps = [small, large, small, large, small]
    x = rnd_f(sum(caps) - 66 * (len(caps) - 1), 0x5EED0053)      # (63 ... 66 samples stay in the window after every call)
    kw = {"translate": translate} if translate else {}
    g = drive_schedule([rr.HilbertFir(31, taps, 4, **kw)], x, caps)
    small_fam = g.fams[0]
    assert small_fam in ("direct", "two-stage"), g.fams
    check_families(g, [small_fam, "prune", small_fam, "prune", small_fam], f"HilbertFir 31 (*) 64 taps /4 {translate}, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.Hilbert(31), orc.FirFilter(taps, deci=4, **kw)], x, takes=g.takes)
    assert all(c[0][:3] == (AGAIN, t, t) for c, t in zip(o.log, g.takes))          # the oracle's Hilbert: everything, at once
    check_filter(g, o, lambda c: c[-1], f"HilbertFir {'translate ' if translate else ''}prune <-> {small_fam}")


# ---- non-finite verdicts across a switch --------------------------------------------------------------------------------
NAN_KINDS = [complex(np.nan, 0.25), complex(-0.5, np.nan), complex(np.nan, np.nan)]


def nan_positions(caps, S, L, layout):
    """Input positions for the four switches of a five-call stream (small -> large, large -> small, twice).  E = the input
    position where a call ends, b = the reference's last block that call emits: its poisoned stretch [b S, (b + 1) S + L)
    reaches L outputs into the next call, which another family runs.
      layout "block":  switches 0, 1: the middle of block b;          switches 2, 3: (b + 1) S - 1, the last sample of block b
      layout "edge":   switches 0, 1: (b + 1) S, the first sample behind block b's edge (a pending sample: block b + 1 is the
                       next call's first);   switches 2, 3: E - 1 and E - L + 1, in the last L samples before the switch
    One placement per switch: two at one switch would poison the same blocks and hide each other."""
    ends = np.cumsum(caps)[:-1]
    pos = []
    for k, E in enumerate(int(e) for e in ends):
        b = E // S - 1
        assert E % S >= 1 and b >= 1                              # (a pending sample exists; block b lies in this call)
        if layout == "block":
            pos += [b * S + S // 2] if k < 2 else [(b + 1) * S - 1]
        else:
            pos += [(b + 1) * S] if k < 2 else [E - 1, E - L + 1]
    return pos


def poison(x, pos):
    x = x.copy()
    for k, p in enumerate(pos):
        x[p] = NAN_KINDS[k % 3]
    return x


def first_outputs_of_next_calls(run):
    """output index of the first sample every call but the first emitted"""
    return np.cumsum([c[-1][2] for c in run.log])[:-1]


@pytest.mark.parametrize("layout", ["block", "edge"])
def test_nan_verdicts_cross_fm_chain_switch(rr, cus, layout):
    """FmChain 463 taps 1:6, full <-> poly, NaN samples (whole and single components) around every switch: the verdict slots a
    call leaves (last block, second-to-last, the carried r) are read by a call of the other family, whose probe stride is its
    own.  The NaN set is the oracle's, and it does reach across every switch; the finite outputs keep the chain bar."""
    taps = TAPS463()
    small, large = fm_windows_1_6(cus)
    caps = [small, large, small, large, small]
    x = poison(station(sum(caps)), nan_positions(caps, 561, 463, layout))
    g = drive_schedule([rr.FmChain(taps, 1, 6, 1.0)], x, caps)
    check_families(g, ["full", "poly", "full", "poly", "full"], f"FmChain NaN {layout}, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps), orc.RationalResampler(1, 6), orc.QuadratureDemod(1.0)], x, caps, keep=1)
    assert not np.isfinite(o.y[first_outputs_of_next_calls(o)]).any()         # every stretch crosses its switch
    check_chain(g, o, fused_view, len(taps), 6, f"FmChain NaN {layout}", nan=True)


@pytest.mark.parametrize("layout", ["block", "edge"])
def test_nan_verdicts_cross_fftfilter_switch(rr, cus, layout):
    """FftFilter 2467 taps, alt <-> split, the same placements: the carried verdict on a call's last reference block (d_tail)
    is written behind one tile size and read behind the other"""
    taps = (rnd_c(2467, 43) / 1000).astype(np.complex64)
    blk = rr.FftFilter(taps)
    S, small, large = filter_windows(rr, blk, 2467, cus)
    caps = [small, large, small, large, small]
    x = poison(noise_c(sum(caps)), nan_positions(caps, S, 2467, layout))
    g = drive_schedule([blk], x, caps)
    check_families(g, ["alt", "split", "alt", "split", "alt"], f"FftFilter NaN {layout}, {cus} CUs, windows {caps}")
    o = drive_schedule([orc.FftFilter(taps)], x, caps)
    assert not np.isfinite(o.y[first_outputs_of_next_calls(o)]).any()
    check_filter(g, o, fused_view, f"FftFilter NaN {layout}", nan=True)
