"""GPU: rr.FskTx (rr_fsk_tx_*, kernels_tx.hip) against the long-double truths and the three bounds of tests/fsk_model.py: both modes,
the issue's ratios, bit patterns and lengths around the audio and the output tile, large steps, the second chunk of the tile-level
scans, splits into pushes, launch counts, refusals, and rr_fm_tx fed the block's own audio."""
import math

import numpy as np
import pytest
import torch

import fsk_dev as fd
import fsk_model as fk
import rustradio_amd as rr
import tx_model as tm

pytestmark = pytest.mark.gpu

K1, K2 = 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
SHAPES = [(10, 1, 4, 1), (40, 1, 25, 24), (3, 7, 3, 7), (1, 1, 1, 1), (7, 3, 4099, 1)]
IDS = [f"{a}:{b}-{c}:{d}" for a, b, c, d in SHAPES]
FULL = 300_000                                # outputs up to which every one is judged; beyond, the subset of _subset()


def make(mode, sh, lo=1200.0, hi=2200.0, k1=K1, gain=0.5, k2=K2):
    return rr.FskTx(mode, sh[0], sh[1], lo, hi, k1, gain, sh[2], sh[3], k2)


def dims():
    return make(rr.FSK_TX_AFSK, SHAPES[0]).dims()


def _bits_for(target, count_of):
    """the bit counts whose count_of(n) (non-decreasing in n) is the largest <= target and the smallest >= target"""
    lo, hi = 0, 1
    while count_of(hi) < target:
        hi *= 2
    while lo < hi:                             # smallest n with count_of(n) >= target
        mid = (lo + hi) // 2
        lo, hi = (mid + 1, hi) if count_of(mid) < target else (lo, mid)
    return {n for n in (lo, lo - 1) if n >= 1}


def bit_counts(sh, atile, otile):
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    A = lambda n: fk.made(n, *r1)
    O = lambda n: fk.made(A(n), *r2)
    ns = {1, 2}
    for t in (atile - 1, atile, atile + 1, 3 * atile + 17):
        ns |= _bits_for(t, A)
    for t in (otile - 1, otile, otile + 1, 3 * otile + 17):
        ns |= _bits_for(t, O)
    return sorted(ns)


def _subset(no, na, r2, atile, seed):
    """outputs judged when there are more than FULL: both ends, 100000 drawn, and the first and last output of the audio runs on
    either side of every audio tile's edge"""
    rng = np.random.default_rng(seed)
    parts = [np.arange(4096), np.arange(no - 4096, no), rng.integers(0, no, 100_000)]
    m = np.concatenate([np.arange(t - 2, t + 2) for t in range(atile, na, atile)] + [np.arange(0)]).astype(np.int64)
    m = m[(m >= 0) & (m < na)]
    f = -((-m * r2[0]) // r2[1])
    f1 = -((-(m + 1) * r2[0]) // r2[1])
    parts += [f, f1 - 1]
    sel = np.unique(np.concatenate(parts).astype(np.int64))
    return sel[(sel >= 0) & (sel < no)]


def judge(mode, sh, tx, bits, out_t, aud_t, atile, label, seed=0):
    """-> the used fraction of the bound (asserted <= 1, the truths' own errors asserted <= 1 % of it); out_t / aud_t on the device"""
    lo, hi, k1, gain, k2 = tx
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    na, no = fk.made(len(bits), *r1), len(out_t)
    sel = None if no <= FULL else _subset(no, na, r2, atile, seed)
    out = (out_t if sel is None else out_t[torch.from_numpy(sel).cuda()]).cpu().numpy()
    if mode == rr.FSK_TX_AFSK:
        audio = aud_t.cpu().numpy()
        assert len(audio) == na
        ua, ta = fk.used_audio(audio, bits, r1, lo, hi, k1, gain)
        uo, to = fk.used_out(out, audio, r2, k2, sel)
    else:
        ua, ta = fk.used_direct(out, na, bits, r1, r2, lo, hi, k1, gain, sel)
        uo, to = 0.0, 0.0
    print(f"{label}: audio {na} out {no}: used {ua:.4f} (stage 1 / DIRECT) {uo:.4f} (AFSK out); truths' own {ta:.1e} {to:.1e}")
    assert ta <= 0.01 and to <= 0.01, label
    assert ua <= 1.0 and uo <= 1.0, label
    return max(ua, uo)


def test_dims():
    assert dims() == (2048, 2048, 4096)


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_bounds(sh, mode):
    """random bits at every length (1, 2, and what puts the audio or the output length at tile - 1, tile, tile + 1, 3 tile + 17, or
    as near as the ratio lets a push come from either side); all-0, all-1 and alternating at the lengths around the audio tile"""
    atile, otile, _ = dims()
    tx = (1200.0, 2200.0, K1, 0.5, K2)
    worst, ns = 0.0, bit_counts(sh, atile, otile)
    r1 = fk.reduced(sh[0], sh[1])
    near = [n for n in ns if atile - 12 <= fk.made(n, *r1) <= atile + 12]
    for n in ns:
        pats = fk.patterns(n, 100 + n)
        for name in ["random"] + (["zeros", "ones", "alt"] if n in near or n <= 2 else []):
            h = make(mode, sh, *tx)
            out, aud, _ = fd.dev_push(h, pats[name], audio=mode == rr.FSK_TX_AFSK)
            worst = max(worst, judge(mode, sh, tx, pats[name], out, aud, atile, f"{name} n={n}", seed=n))
    print(f"worst used fraction of the bound: {worst:.4f}")


@pytest.mark.parametrize("which", ["k1", "k2", "k1-direct"])
def test_large_steps(which):
    """|k1 hi| > 4 pi and |k2 gain| > 4 pi, judged by the same formulas (the bound's d1 / d2 term carries them)"""
    atile, _, _ = dims()
    sh, n = (10, 1, 4, 1), 3 * 205 + 7
    bits = fk.patterns(n, 9)["random"]
    mode = rr.FSK_TX_DIRECT if which.endswith("direct") else rr.FSK_TX_AFSK
    tx = {"k1": (-1.0, 1.0, 14.2, 0.5, K2), "k2": (1200.0, 2200.0, K1, 0.5, 9.5 * math.pi),
          "k1-direct": (-1.0, 1.0, -14.2, 2.0, 0.0)}[which]
    assert (abs(tx[2] * tx[1]) > 4 * math.pi) if which != "k2" else (abs(tx[4] * tx[3]) > 4 * math.pi)
    h = make(mode, sh, *tx)
    out, aud, _ = fd.dev_push(h, bits, audio=mode == rr.FSK_TX_AFSK)
    u = judge(mode, sh, tx, bits, out, aud, atile, which)
    print(f"worst used fraction of the bound: {u:.4f}")


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
def test_second_scan_chunk(mode):
    """more audio tiles than one pass of the tile-level scans takes (1:1 / 1:1, so the outputs are as many): stage 1 against the
    counts' exact phase, stage 2 against the long-double sum over the push's own audio whose carry is reduced every few hundred
    terms; both truths' own errors at most 1 % of the bound; the outputs judged are those of fsk_model's subset, which holds the
    last 4096 and the runs on either side of every audio tile's edge"""
    atile, _, chunk = dims()
    sh, n = (1, 1, 1, 1), atile * chunk + 5000
    bits = fk.patterns(n, 77)["random"]
    tx = (-1.0, 2.0, 0.37, 0.5, 0.61)
    h = make(mode, sh, *tx)
    out, aud, nl = fd.dev_push(h, bits, audio=mode == rr.FSK_TX_AFSK)
    assert nl == (5 if mode == rr.FSK_TX_AFSK else 4)
    u = judge(mode, sh, tx, bits, out, aud, atile, "second chunk", seed=4)
    print(f"worst used fraction of the bound: {u:.4f}")
    # stage 1 once more, against tx_model.vco_truth_grid on the integer levels (g = 0): a plain long-double cumsum is not exact here
    q = np.where(bits != 0, 2, -1).astype(np.int64)
    truth = tm.vco_truth_grid(q, 0, tx[2])
    b = fk.audio_bound(np.arange(n), tx[3], fk.d1_of(*tx[:3]))
    assert tx[3] * tm.truth_grid_error(n, tx[2], 0, 2) <= 0.01 * float(b[0])
    if mode == rr.FSK_TX_AFSK:
        err = np.abs(aud.cpu().numpy().astype(np.float64) - tx[3] * truth.real)
    else:
        o = out.cpu().numpy()
        err = np.maximum(np.abs(o.real.astype(np.float64) - tx[3] * truth.real), np.abs(o.imag.astype(np.float64) - tx[3] * truth.imag))
    print(f"stage 1 against vco_truth_grid: used {float(np.max(err / b)):.4f}")
    assert np.all(err <= b)


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
@pytest.mark.parametrize("sh", SHAPES[:4], ids=IDS[:4])
def test_splits(sh, mode):
    """one stream whole and in random splits with 1-bit and empty pushes: equal counts, both within the bound (each against the
    truth from the stream's start; AFSK out against its OWN audio), nothing written at or beyond the counts (fsk_dev.dev_push),
    the same pushes twice the same bits, and out the same bits with and without d_audio"""
    atile, _, _ = dims()
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    n = max(8, (2 * atile + 300) * r1[1] // r1[0])
    bits = fk.patterns(n, 21)["random"]
    tx = (1200.0, 2200.0, K1, 0.5, K2)
    afsk = mode == rr.FSK_TX_AFSK
    whole_o, whole_a, _ = fd.run_pushes(make(mode, sh, *tx), bits, [n], audio=afsk)
    rng = np.random.default_rng(n)
    for k in (3, 9):
        sp = fk.splits(rng, n, k)
        o, a, _ = fd.run_pushes(make(mode, sh, *tx), bits, sp, audio=afsk)
        o2, a2, _ = fd.run_pushes(make(mode, sh, *tx), bits, sp, audio=afsk)
        assert fd.same_bits(o, o2) and (not afsk or fd.same_bits(a, a2))
        assert len(o) == len(whole_o) == fk.made(fk.made(n, *r1), *r2)
        judge(mode, sh, tx, bits, torch.from_numpy(o), torch.from_numpy(a) if afsk else None, atile, f"{k} cuts")
        if afsk:
            o3, _, _ = fd.run_pushes(make(mode, sh, *tx), bits, sp, audio=False)
            assert fd.same_bits(o, o3)
    judge(mode, sh, tx, bits, torch.from_numpy(whole_o), torch.from_numpy(whole_a) if afsk else None, atile, "whole")


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
def test_launch_counts(mode):
    """the numbers of kernels_tx.hip's header, whatever the bits: 2 for a push of one audio tile, 5 (AFSK) / 4 (DIRECT) beyond, one
    fewer where the push has audio but no output, 0 for an empty push and for bits that make no audio sample"""
    atile, _, _ = dims()
    many = 5 if mode == rr.FSK_TX_AFSK else 4
    afsk = mode == rr.FSK_TX_AFSK
    for name in ("zeros", "ones", "alt", "random"):
        h = make(mode, (10, 1, 4, 1))
        nls = []
        for n in (1, atile // 10, atile // 10 + 1, 3 * atile // 10 + 17, 0):
            nls.append(fd.dev_push(h, fk.patterns(n, 5)[name], audio=afsk)[2])
        assert nls == [2, 2, many, many, 0], name
    h = make(mode, (3, 7, 1, 4099))
    seq = [fd.dev_push(h, fk.patterns(n, 6)["random"], audio=afsk) for n in (1, 1, 1, 7 * atile)]
    # bit 0 makes audio sample 0 and output 0; bit 1 makes no audio sample; bit 2 makes audio sample 1, which the second resampler drops
    assert [(len(q[0]), q[2]) for q in seq[:3]] == [(1, 2), (0, 0), (0, 1)]
    assert seq[3][2] == many


def test_push_refusals_launch_nothing_and_change_nothing():
    atile, _, _ = dims()
    sh, n = (10, 1, 4, 1), 300
    bits = fk.patterns(2 * n, 31)["random"]
    tx = (1200.0, 2200.0, K1, 0.5, K2)
    h = make(rr.FSK_TX_AFSK, sh, *tx)
    o1, a1, _ = fd.run_pushes(h, bits[:n], [n])
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, big = d.data_ptr(), 1 << 40
    l0 = fd.launches()
    for args, msg in [((0, n, p, big, 0, 0), "null bit buffer"), ((p, n, 0, big, 0, 0), "null output buffer"),
                      ((p, n, p, 40 * n - 1, 0, 0), "out_cap below"), ((p, n, p, big, p, 10 * n - 1), "audio_cap below"),
                      ((p, (1 << 30) + 1, p, big, 0, 0), "more than 2\\^30 bits"),
                      ((p, 1 << 28, p, big, 0, 0), "more than 2\\^30 audio samples"),
                      ((p, 1 << 25, p, big, 0, 0), "more than 2\\^30 outputs")]:
        with pytest.raises(ValueError, match=msg):
            h.push_dev(*args)
    with pytest.raises(ValueError, match="more than 2\\^30 outputs"):
        h.count(1 << 25)
    hd = make(rr.FSK_TX_DIRECT, sh, *tx)
    with pytest.raises(ValueError, match="DIRECT mode has no audio output"):
        hd.push_dev(p, n, p, big, p, big)
    assert fd.launches() == l0
    assert h.push_dev(0, 0, 0, 0, 0, 0) == (0, 0) and fd.launches() == l0           # (an empty push needs no buffers)
    o2, a2, _ = fd.run_pushes(h, bits[n:], [n])
    wo, wa, _ = fd.run_pushes(make(rr.FSK_TX_AFSK, sh, *tx), bits, [n, n])
    assert fd.same_bits(np.concatenate([o1, o2]), wo) and fd.same_bits(np.concatenate([a1, a2]), wa)
    with pytest.raises(RuntimeError, match="FskTx takes pushes of line bits"):          # rr_block_work on the handle is an error
        h.work(np.zeros(4, np.uint8), 16)


def test_host_push_equals_device_push():
    sh, n = (10, 1, 4, 1), 700
    bits = fk.patterns(n, 41)["random"]
    o, a = make(rr.FSK_TX_AFSK, sh).push(bits, audio=True)
    wo, wa, _ = fd.run_pushes(make(rr.FSK_TX_AFSK, sh), bits, [n])
    assert fd.same_bits(o, wo) and fd.same_bits(a, wa)
    od = make(rr.FSK_TX_DIRECT, sh).push(bits)
    wd, _, _ = fd.run_pushes(make(rr.FSK_TX_DIRECT, sh), bits, [n], audio=False)
    assert fd.same_bits(od, wd)
    assert len(make(rr.FSK_TX_AFSK, sh).push([])) == 0


@pytest.mark.parametrize("sh", [(10, 1, 4, 1), (40, 1, 25, 24), (3, 7, 3, 7)], ids=IDS[:3])
def test_against_fm_tx_over_the_blocks_own_audio(sh):
    """rr_fm_tx(I2, D2, k2) fed the audio this block wrote: the same work done by a scan at the output rate.  Both are within
    bound_steps of the same truth, so they are within twice the bound of each other."""
    atile, _, _ = dims()
    r1 = fk.reduced(sh[0], sh[1])
    n = max(8, (2 * atile + 300) * r1[1] // r1[0])
    bits = fk.patterns(n, 51)["random"]
    out, aud, _ = fd.dev_push(make(rr.FSK_TX_AFSK, sh), bits)
    na, no = len(aud), len(out)
    ref = torch.zeros(no + 64, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    fm = rr.FmTx(sh[2], sh[3], K2)
    _, consumed, produced, _ = fm.work_dev(aud.data_ptr(), na, ref.data_ptr(), no + 64)
    fm.sync()
    assert consumed == na and produced == no
    got, want = out.cpu().numpy(), ref[:no].cpu().numpy()
    d2 = abs(K2) * float(np.max(np.abs(aud.cpu().numpy())))
    b = 2.0 * fk.out_bound(np.arange(no), d2)
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag))
    print(f"against rr_fm_tx: used {float(np.max(err / b)):.4f} of twice the bound")
    assert np.all(err <= b)
