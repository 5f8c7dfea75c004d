"""GPU: rr_bit_decoder and the single bit blocks (kernels_bits.hip) over drawn configurations — every stage on and off, random
descramblers up to length 63, codes of every length class around the 32 / 33 switch, allowed differences from 0 to far above
64 — fed in one call, in many (70 one-sample calls first) and through misaligned device windows; the slicer's special values
inside the fused block and inside the history a later tile reads again; and bytes other than 0 / 1 into the u8 blocks.
Every comparison is bit for bit against bits_model.Chain, the sequential state machines.  tests/test_bits_cpu.py holds the
generator below to its own conditions without a GPU."""
import numpy as np
import pytest

import rustradio_amd as rr
from bits_model import G3RUH, HDLC_FLAG, Chain, Lfsr, Nrzi, Slide, slicer
from test_gpu_bits import T, cut_windows, feed, run_whole, tag_pairs
from tx_model import sync_rule

pytestmark = pytest.mark.gpu

SEEDS = range(48)
DESCRAMBLER_LENS = [0, 1, 5, 16, 31, 62, 63]
CODE_LENS = [1, 3, 7, 8, 24, 31, 32, 33, 40, 63, 64]
OFFSETS = [0, 1, 3, 5, 16]
ONES_FIRST = 70                       # one-sample calls at the start of the split feed: `seen` is carried past 64
_FULL64 = (1 << 64) - 1
_FORCED = {                           # the corners the draw must not miss
    0: dict(invert=False, nrzi=True, descrambler=(_FULL64, (1 << 63) | 5, 63), L=64, allowed=0),
    1: dict(invert=True, nrzi=True, descrambler=(0x8000000000000001, 1, 63), L=33, allowed=3),
    2: dict(invert=False, nrzi=True, descrambler=G3RUH, L=32, allowed=1),
    3: dict(invert=True, nrzi=False, descrambler=None, L=40, allowed=2 ** 40),
    4: dict(invert=False, nrzi=False, descrambler=None, L=31, allowed=31),
    5: dict(invert=False, nrzi=False, descrambler=(0x5A5A5A5A5A5A5A5A, 0x2BCDEF0123456789, 62), L=0, allowed=0),
    6: dict(invert=True, nrzi=True, descrambler=(0x80000021, 0xFFFFFFFF, 31), L=63, allowed=63),
    7: dict(invert=False, nrzi=False, descrambler=(1, 1, 0), L=8, allowed=0),
}
_CASES = {}


def unscramble_inverse(s, mask, seed, length):
    """the d with Lfsr(mask, seed, length).run(d) == s: the register is fed by d, so d[n] = s[n] ^ parity(reg & mask)"""
    reg, out = int(seed), []
    for v in s:
        d = int(v) ^ (bin(reg & mask).count("1") & 1)
        reg = (reg >> 1) | (d << length)
        out.append(d)
    return out


def nrzi_inverse(d):
    """the r with Nrzi().run(r) == d: r[n] = 1 ^ d[n] ^ r[n-1], r[-1] = 0"""
    last, out = 0, []
    for v in d:
        last = 1 ^ int(v) ^ last
        out.append(last)
    return out


def draw_config(rng, seed):
    if seed in _FORCED:
        return dict(_FORCED[seed])
    if rng.random() < 0.25:                                                        # one stage alone: the u8 single blocks too
        cfg = dict(invert=False, nrzi=False, descrambler=None, L=0, allowed=0)
        one = int(rng.integers(3))
        if one == 0:
            cfg["nrzi"] = True
            return cfg
    else:
        cfg, one = dict(invert=bool(rng.integers(2)), nrzi=bool(rng.integers(2)), descrambler=None, L=0, allowed=0), None
    if one in (None, 1):
        kind = int(rng.integers(3)) if one is None else 1 + int(rng.integers(2))
        if kind == 1:
            cfg["descrambler"] = G3RUH
        elif kind == 2:
            length = DESCRAMBLER_LENS[int(rng.integers(len(DESCRAMBLER_LENS)))]
            full = (2 << length) - 1
            mask = int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(4))
            if rng.random() < 0.5:
                mask &= full                                                       # (otherwise: bits above len, which change nothing)
            cfg["descrambler"] = (mask & _FULL64, (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(4))) & full, length)
    if one in (None, 2) and (one == 2 or rng.random() < 0.85):
        L = CODE_LENS[int(rng.integers(len(CODE_LENS)))]
        cfg["L"], cfg["allowed"] = L, [0, 1, 3, L, 2 ** 40][int(rng.integers(5))]
    return cfg


def fuzz_case(seed):
    """-> the case of a seed, made once and never modified: the configuration, the soft stream x that decodes to the drawn
    bits `s` with the code planted in them, the windows of the split feed, the calls and offsets of the device feed, and
    what Chain makes of x (`bits`, `tags` stream-relative)"""
    if seed in _CASES:
        return _CASES[seed]
    rng = np.random.default_rng(9000 + seed)
    cfg = draw_config(rng, seed)
    L, allowed = cfg["L"], cfg["allowed"]
    if seed in _FORCED:
        n = int(rng.integers(2 * T + 500, 3 * T + 201))
    elif seed % 4 == 1:
        n = int(rng.integers(1, 201))                                              # shorter than the history, some shorter than the code
    else:
        n = int(rng.integers(1, 3 * T + 201))
    code = rng.integers(0, 2, L).tolist() if L else None
    s = rng.integers(0, 2, n).tolist()
    head = min(ONES_FIRST, n)
    cut = int(rng.integers(head + 2 * L + 1, n)) if n > head + 2 * L + 1 else None   # the call cut a planted code straddles
    if cut is not None and abs(cut - T) < 200 and cut + 400 < n:
        cut += 400                                                                 # (clear of the one planted across the tile seam)
    plants = []
    if L:
        for start in (0, T - L // 2, None if cut is None else cut - (L + 1) // 2):
            if start is None or start < 0 or start + L > n or any(abs(start - p) < L for p in plants):
                continue
            word = list(code)
            for k in rng.permutation(L)[:int(rng.integers(0, min(allowed, L) + 1))]:
                word[k] ^= 1                                                       # up to `allowed` differences: still a match
            s[start:start + L] = word
            plants.append(start)
    r = s
    if cfg["descrambler"] is not None:
        r = unscramble_inverse(r, *cfg["descrambler"])
    if cfg["nrzi"]:
        r = nrzi_inverse(r)
    r = np.array(r, np.uint8)
    line = r ^ np.uint8(1) if cfg["invert"] else r
    x = ((2.0 * line - 1.0) * rng.uniform(0.2, 1.5, n)).astype(np.float32)
    # the split feed: one-sample calls, then windows that end at the cut and at a few other places
    cuts = sorted({c for c in ([cut] if cut else []) + rng.integers(1, n + 1, 3).tolist() + [T + 1, 2 * T + 100] if head < c < n})
    windows = [(1, 1)] * head + (cut_windows(n - head, [c - head for c in cuts], 300 + seed) if n > head else [])
    # the device feed: two or three calls, each with its own input element offset and output byte offset
    ends = sorted(set(rng.integers(1, n + 1, int(rng.integers(1, 3))).tolist()) | {n})
    dev = [(a, b, OFFSETS[int(rng.integers(5))], OFFSETS[int(rng.integers(5))]) for a, b in zip([0] + ends[:-1], ends)]
    bits, pos, diffs = Chain(invert=cfg["invert"], nrzi=cfg["nrzi"], descrambler=cfg["descrambler"], code=code,
                             allowed_diffs=allowed).run(x)
    stages = [k for k in ("nrzi", "descrambler", "L") if cfg[k]]
    case = dict(cfg, seed=seed, n=n, code=code, s=np.array(s, np.uint8), r=r, x=x, plants=plants, cut=cut, windows=windows, dev=dev,
                bits=bits, tags=list(zip(pos.tolist(), diffs.tolist())),
                single=stages[0] if len(stages) == 1 and not cfg["invert"] else None)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[seed] = case
    return case


def moving_calls(windows, n):
    """the [start, end) of every call of a feed that moves samples"""
    pos, out = 0, []
    for w, cap in windows:
        m = min(w, cap, n - pos)
        if m > 0:
            out.append((pos, pos + m)); pos += m
    assert pos == n
    return out


def make_fused(c):
    return rr.BitDecoder(invert=c["invert"], nrzi=c["nrzi"], descrambler=c["descrambler"], code=c["code"], allowed_diffs=c["allowed"])


def make_single(c):
    if c["single"] == "nrzi":
        return rr.NrziDecode()
    if c["single"] == "descrambler":
        return rr.Descrambler(*c["descrambler"])
    return rr.CorrelateAccessCodeTag(c["code"], c["allowed"])


def blocks_of(c):
    """(block factory, its source) — the fused block on the soft stream and, for a configuration that is one stage, the u8
    single block on the sliced bits"""
    return [(make_fused, c["x"])] + ([(make_single, c["r"])] if c["single"] else [])


# ---- C1. configuration fuzz -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_config_fuzz_one_call(seed):
    c = fuzz_case(seed)
    for make, src in blocks_of(c):
        blk = make(c)
        assert np.array_equal(run_whole(blk, src), c["bits"]), (seed, blk.name)
        if c["code"]:
            assert tag_pairs(blk) == c["tags"], (seed, blk.name)


@pytest.mark.parametrize("seed", SEEDS)
def test_config_fuzz_split(seed):
    c = fuzz_case(seed)
    for make, src in blocks_of(c):
        blk = make(c)
        y, t = feed(blk, src, c["windows"], tagged=bool(c["code"]))
        assert np.array_equal(y, c["bits"]) and t == c["tags"], (seed, blk.name)


@pytest.mark.parametrize("seed", SEEDS)
def test_config_fuzz_device_windows(seed):
    import torch
    c = fuzz_case(seed)
    for make, src in blocks_of(c):
        blk, tags, f32 = make(c), [], src.dtype == np.float32
        for a, b, in_off, out_off in c["dev"]:
            m = b - a
            d_in = torch.zeros(m + 32, dtype=torch.float32 if f32 else torch.uint8, device="cuda")
            d_out = torch.full((m + 64,), 9, dtype=torch.uint8, device="cuda")
            d_in[in_off:in_off + m] = torch.from_numpy(src[a:b].copy()).cuda()
            assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            assert blk.work_dev(d_in.data_ptr() + in_off * src.itemsize, m, d_out.data_ptr() + out_off, m) == sync_rule(m, m)
            blk.sync()
            if c["code"]:
                tags += [(a + p, d) for p, d in tag_pairs(blk)]
            got = d_out.cpu().numpy()
            assert np.array_equal(got[out_off:out_off + m], c["bits"][a:b]), (seed, blk.name, a, b, in_off, out_off)
            assert np.all(got[:out_off] == 9) and np.all(got[out_off + m:] == 9)   # nothing outside the window is written
        assert tags == c["tags"], (seed, blk.name)


# ---- C2. the slicer's special values inside the fused block ----------------------------------------------------------------------
def special_values():
    f = np.finfo(np.float32)
    return np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, f.smallest_subnormal, f.tiny, -f.tiny, f.max, -f.max],
                    np.float32)


@pytest.mark.parametrize("in_off", [0, 1], ids=["aligned", "one-element-off"])
@pytest.mark.parametrize("invert", [False, True])
def test_slicer_specials_in_the_fused_block(invert, in_off):
    import torch
    vals = special_values()
    n = 2 * T + 333
    x = np.resize(vals, n)
    for lo in (T - 128, 2 * T - 128):                                              # the history a later tile loads again
        seen = {int(i) % 13 for i in range(lo, lo + 128)}
        assert seen == set(range(13)) and np.isnan(x[lo:lo + 128]).sum() >= 18
    assert slicer(x[:13]).tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0]
    want_bits, pos, diffs = Chain(invert=invert, nrzi=True, descrambler=G3RUH, code=HDLC_FLAG).run(x)
    if invert:                                                                     # a NaN slices to 0, and invert makes it 1
        assert Chain(invert=True).run(x[:2])[0].tolist() == [1, 1]
    d_in = torch.zeros(n + 16, dtype=torch.float32, device="cuda")
    d_out = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + n] = torch.from_numpy(x).cuda()
    blk = rr.BitDecoder(invert=invert, nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    torch.cuda.synchronize()
    first = T + 77                                                                 # two calls: the specials in the carried state too
    assert blk.work_dev(d_in.data_ptr() + 4 * in_off, first, d_out.data_ptr(), first) == sync_rule(first, first)
    tags = tag_pairs(blk)
    assert blk.work_dev(d_in.data_ptr() + 4 * (in_off + first), n - first, d_out.data_ptr() + first, n - first) == sync_rule(n - first, n - first)
    tags += [(first + p, d) for p, d in tag_pairs(blk)]
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:n], want_bits) and np.all(got[n:] == 9)
    assert tags == list(zip(pos.tolist(), diffs.tolist()))
    # and as host windows through work(), one call
    blk = rr.BitDecoder(invert=invert, nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    assert np.array_equal(run_whole(blk, x), want_bits) and tag_pairs(blk) == tags


# ---- C3. bytes other than 0 / 1: the lowest bit only --------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 3)], ids=["aligned", "offsets-1-3"])
@pytest.mark.parametrize("which", ["nrzi", "descrambler", "correlator"])
def test_u8_blocks_read_the_lowest_bit_only(which, in_off, out_off):
    import torch
    rng = np.random.default_rng(70)
    n = 2 * T + 333
    low = rng.integers(0, 2, n).astype(np.uint8)
    low[T - 4:T + 4] = HDLC_FLAG
    low[100:108] = HDLC_FLAG
    dirty = low | (rng.integers(0, 128, n).astype(np.uint8) << 1)
    dirty[:64] = low[:64] | 0xFE                                                   # every high bit set ...
    dirty[64:128] = low[64:128]                                                    # ... and none
    assert np.array_equal(dirty & 1, low) and np.count_nonzero(dirty > 1) > n * 0.9
    if which == "nrzi":
        blk, want, tags = rr.NrziDecode(), np.array(Nrzi().run(low), np.uint8), None
    elif which == "descrambler":
        blk, want, tags = rr.Descrambler.g3ruh(), np.array(Lfsr(*G3RUH).run(low), np.uint8), None
    else:                                                                          # the pass-through delivers in & 1 as well
        blk, want, tags = rr.CorrelateAccessCodeTag(HDLC_FLAG, 1), low, Slide(HDLC_FLAG, 1).run(low)
        assert (107, 0) in tags and (T + 3, 0) in tags
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + n] = torch.from_numpy(dirty).cuda()
    torch.cuda.synchronize()
    first, got_tags = T + 1001, []
    for a, b in ((0, first), (first, n)):
        assert blk.work_dev(d_in.data_ptr() + in_off + a, b - a, d_out.data_ptr() + out_off + a, b - a) == sync_rule(b - a, b - a)
        blk.sync()
        if tags is not None:
            got_tags += [(a + p, d) for p, d in tag_pairs(blk)]
    got = d_out.cpu().numpy()
    assert np.all(got[:out_off] == 9) and np.all(got[out_off + n:] == 9)
    assert got[out_off:out_off + n].max() <= 1                                     # every output byte is 0 or 1
    assert np.array_equal(got[out_off:out_off + n], want)
    assert tags is None or got_tags == tags
    # host windows (aligned staging buffers), one call
    blk2 = type(blk)(HDLC_FLAG, 1) if tags is not None else (rr.NrziDecode() if which == "nrzi" else rr.Descrambler.g3ruh())
    y = run_whole(blk2, dirty)
    assert y.max() <= 1 and np.array_equal(y, want) and (tags is None or tag_pairs(blk2) == tags)
