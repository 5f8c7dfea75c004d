"""GPU: Vco and FmTx past one pass of their loops.  A window of more than 8 tiles per CU sends the workgroups of k_vco_sums /
k_vco_apply round their grid-stride loops a second time; one of more than VCO_SB * VCO_SPER tiles sends k_vco_scan into a
second chunk, which takes its base from the first.  The inputs lie on a dyadic grid, so the truth is exact up to one long-double
product (tests/tx_model.py vco_truth_grid) and the bound is the one the small cases are held to."""
import math
import os
import re

import numpy as np
import pytest
import torch

import rustradio_amd as rr
from harness import WAIT_DST, WAIT_SRC
from tx_model import (GRID_G, bound, comp_err, fm_tx_truth_grid, grid_noise, grid_signal, sync_rule, truth_grid_error,
                      vco_truth_grid)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 2048                              # VCO_T: samples of a scan tile
SB, SPER = 1024, 4                    # VCO_SB, VCO_SPER: k_vco_scan's threads and tile sums per thread
CH = SB * SPER                        # tile sums of one chunk of k_vco_scan
PER_CU = 8                            # tiles_grid (packet_common.hpp): at most this many workgroups per CU
K75 = 2.0 * math.pi * 75000 / 480000

_HEAD, _TAIL1, _TAIL2 = 3 * T + 17, 700, T + 5     # the calls around the big window
_SEED = 31


def grid_cap():
    """the cap of tiles_grid: a window of more tiles than this sends workgroups round their loops again"""
    return PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


def big_lengths():
    G = grid_cap()
    return {"G*T+1": G * T + 1, "CH*T": CH * T, "CH*T+1": CH * T + 1, "(CH+1)*T+17": (CH + 1) * T + 17,
            "2*CH*T+5*T+3": 2 * CH * T + 5 * T + 3}


_LENGTHS = ["G*T+1", "CH*T", "CH*T+1", "(CH+1)*T+17", "2*CH*T+5*T+3"]
_NMAX = _HEAD + 2 * CH * T + 5 * T + 3 + _TAIL1 + _TAIL2
_cache = {}


def noise_and_truth():
    """one noise stream for every case of this module and its truth at K75, computed once and never written to: a case of n
    samples takes the first n of both (the truth of a prefix is the prefix of the truth)"""
    if "noise" not in _cache:
        q, a = grid_noise(_NMAX, _SEED)
        t = vco_truth_grid(q, GRID_G, K75)
        for v in (q, a, t):
            v.setflags(write=False)
        _cache["noise"] = (q, a, t)
    return _cache["noise"]


def test_constants_mirror_the_kernel():
    csrc = os.path.join(ROOT, "rustradio_amd", "csrc")
    assert f"constexpr int VCO_T = {T};" in open(os.path.join(csrc, "kernels.hpp")).read()
    src = open(os.path.join(csrc, "kernels_tx.hip")).read()
    assert f"constexpr int VCO_SB = {SB}, VCO_SPER = {SPER}, VCO_SCHUNK = VCO_SB * VCO_SPER;" in src
    assert "const unsigned g = tiles_grid(ntiles);" in src                         # ... of packet_common.hpp:
    grid = open(os.path.join(csrc, "packet_common.hpp")).read()
    grid = grid[grid.index("static inline unsigned tiles_grid("):]
    assert re.search(r"std::min\(ntiles, \(long\)device_cu_count\(\) \* %d\)" % PER_CU, grid[:grid.index("}")])
    assert "for (long c0 = 0; c0 < ntiles; c0 += VCO_SCHUNK)" in src
    assert src.count("tile < ntiles; tile += gridDim.x") == 2


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def within(got, truth, n_bound, k, what):
    e, b = comp_err(got, truth), bound(n_bound)
    print(f"{what}: {len(got)} outputs, worst component error {e:.4e}, bound {b:.4e}")
    assert truth_grid_error(n_bound, k) <= 0.01 * b, "the truth is not exact enough to judge this case"
    assert e <= b, (what, e, b)


# ---- 1. Vco: the grid-stride loops and the scan's chunk loop ----------------------------------------------------------------
# (DC +1 at K75 turns 320 times per tile exactly: every tile sum is 0 modulo 2 pi, so that case sees the drift of 8.4 M
#  additions and nothing of the tile scan.  DC -1 at k = 1 is the same length with tile sums that matter.)
_VCO_CASES = [("noise", K75, w) for w in _LENGTHS] + [("dc+1", K75, "(CH+1)*T+17"), ("dc-1", 1.0, "(CH+1)*T+17")]


@pytest.mark.parametrize("signal,k,which", _VCO_CASES, ids=[f"{s}-{'K75' if k == K75 else k}-{w}" for s, k, w in _VCO_CASES])
def test_vco_many_tiles(signal, k, which):
    big = big_lengths()[which]
    G = grid_cap()
    ntiles = -(-big // T)
    assert ntiles > G, "the window does not reach the grid-stride loop on this device"
    if which in ("CH*T+1", "(CH+1)*T+17", "2*CH*T+5*T+3"):
        assert ntiles > CH, "the window does not reach the second chunk of k_vco_scan"
    n = _HEAD + big + _TAIL1 + _TAIL2
    if signal == "noise":
        _, a, truth = noise_and_truth()
        a, truth = a[:n], truth[:n]
    else:
        q = np.full(n, (1 << GRID_G) if signal == "dc+1" else -(1 << GRID_G), np.int64)
        a, truth = grid_signal(q), vco_truth_grid(q, GRID_G, k)
    blk = rr.Vco(k)
    pos, outs = 0, []
    for m, want in ((_HEAD, 3), (big, 3), (_TAIL1, 1), (_TAIL2, 3)):      # the scratch regrows at the big call
        l0 = launches()
        st, c, p, need, y = blk.work(a[pos:pos + m], m)
        assert launches() - l0 == want, (m, launches() - l0)
        assert (st, c, p, need) == sync_rule(m, m) == (WAIT_SRC, m, m, 1)
        outs.append(y); pos += m
    assert pos == n
    within(np.concatenate(outs), truth, n, k, f"vco {signal} k={k:.6g} {which}={big} ({ntiles} tiles, grid cap {G})")


# ---- 2. a non-finite sample deep inside a many-tile window ---------------------------------------------------------------------
_NF = (CH + 1) * T + 17


def bad_positions():
    return {"G*T": grid_cap() * T, "(CH-1)*T+5": (CH - 1) * T + 5, "CH*T-1": CH * T - 1, "CH*T": CH * T, "n-1": _NF - 1}


@pytest.mark.parametrize("bad,where", [(float("nan"), w) for w in ("G*T", "(CH-1)*T+5", "CH*T-1", "CH*T", "n-1")] +
                         [(float("-inf"), "CH*T")])
def test_vco_non_finite_many_tiles(bad, where):
    p = bad_positions()[where]
    assert 0 < p < _NF and -(-_NF // T) > CH and -(-_NF // T) > grid_cap()
    _, a, truth = noise_and_truth()
    x = a[:_NF].copy()
    x[p] = bad
    blk = rr.Vco(K75)
    st, c, n_out, need, y = blk.work(x, _NF)
    assert (st, c, n_out, need) == sync_rule(_NF, _NF)
    within(y[:p], truth[:p], p, K75, f"before {bad} at {where}={p}")
    later = blk.work(a[_NF:_NF + _TAIL1], _TAIL1)[4]                     # the single-tile kernel on finite input
    assert len(later) == _TAIL1
    for part in (y[p:], later):
        assert len(part) and np.all(np.isnan(part.real)) and np.all(np.isnan(part.imag))


# ---- 3. the fused block over more than one chunk of tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("I,D,n_in,first_cap", [(10, 1, 839_210, 3), (2, 3, 12_586_200, None)])
def test_fm_tx_many_tiles(I, D, n_in, first_cap):
    n_out = -(-n_in * I // D)
    assert n_out == {10: 8_392_100, 2: 8_390_800}[I] and n_out - 3 > (CH + 1) * T
    q, a, _ = noise_and_truth()
    q, a = q[:n_in], a[:n_in]
    blk = rr.FmTx(I, D, K75)
    outs, pos = [], 0
    if first_cap:                                 # 10:1, a window of 3: one sample taken, 7 of its 10 repeats still owed ...
        st, c, p, need, y = blk.work(a, first_cap)
        assert (st, c, p, need) == (WAIT_DST, 1, first_cap, 1)
        outs.append(y); pos = c
    done = sum(len(y) for y in outs)
    st, c, p, need, y = blk.work(a[pos:], n_out + 1)                      # ... and paid first, inside tile 0 of the big call
    assert (st, c, p, need) == (WAIT_SRC, n_in - pos, n_out - done, 1)
    outs.append(y)
    within(np.concatenate(outs), fm_tx_truth_grid(q, GRID_G, I, D, K75, n_out), n_out, K75, f"fm_tx {I}:{D} n_in={n_in}")
