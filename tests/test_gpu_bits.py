"""GPU: rr_binary_slicer / rr_nrzi_decode / rr_descrambler / rr_correlate_access_code_tag and their fusion rr_bit_decoder
(kernels_bits.hip) against the sequential state machines of tests/bits_model.py.  Every comparison is bit for bit: the blocks are
exact in integers, so there is no tolerance anywhere in this file."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import rustradio_amd as rr
from bits_model import G3RUH, HDLC_FLAG, IL2P_SYNC32, Chain, Lfsr, Nrzi, Slide, ax25ish_symbols, chain_vectorised, slicer
from harness import WAIT_DST, WAIT_SRC
from tx_model import sync_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 4096                              # the tile: BITS_T in rustradio_amd/csrc/kernels.hpp


def test_tile_constant_mirrors_the_kernel():
    src = open(os.path.join(ROOT, "rustradio_amd", "csrc", "kernels.hpp")).read()
    assert f"constexpr int BITS_T = {T};" in src


_EDGES = [1, 2, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, T - 1, T, T + 1, 3 * T + 17]
_RANDOM = [int(v) for v in np.random.default_rng(1).integers(1, 5 * T + 1, 20)]
_LENGTHS = _EDGES + _RANDOM
_NMAX = 5 * T

_SHARED = {}


def shared():
    """one soft stream and one bit stream of 5 T samples, and what every single block's model makes of each prefix's source —
    computed once, never modified"""
    if not _SHARED:
        rng = np.random.default_rng(2)
        x = rng.normal(0.0, 1.0, _NMAX).astype(np.float32)
        b = rng.integers(0, 2, _NMAX).astype(np.uint8)
        b[1000:1008] = HDLC_FLAG                  # some certain matches, one across the first tile boundary
        b[T - 3:T + 5] = HDLC_FLAG
        _SHARED.update(x=x, b=b, sliced=slicer(x), nrzi=np.array(Nrzi().run(b), np.uint8),
                       descr=np.array(Lfsr(*G3RUH).run(b), np.uint8), tags=Slide(HDLC_FLAG, 1).run(b))
        for v in _SHARED.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _SHARED


def check_sync_counts(blk, x):
    n = len(x)
    assert blk.work(x, 0)[:4] == sync_rule(n, 0) == (WAIT_DST, 0, 0, 1)
    assert blk.work(x[:0], n)[:4] == sync_rule(0, n) == (WAIT_SRC, 0, 0, 1)


def run_whole(blk, x):
    """one call over all of x -> out"""
    st, c, p, need, y = blk.work(x, len(x))
    assert (st, c, p, need) == sync_rule(len(x), len(x))
    return y


def tag_pairs(blk):
    pos, diffs = blk.tags()
    assert pos.dtype == np.uint64 and diffs.dtype == np.uint8
    return list(zip(pos.tolist(), diffs.tolist()))


# ---- 1. every single block over the lengths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", _LENGTHS)
def test_single_blocks_lengths(n):
    s = shared()
    for make, src, want in ((rr.BinarySlicer, s["x"], s["sliced"]), (rr.NrziDecode, s["b"], s["nrzi"]),
                            (rr.Descrambler.g3ruh, s["b"], s["descr"])):
        blk = make()
        check_sync_counts(blk, src[:n])
        assert np.array_equal(run_whole(blk, src[:n]), want[:n]), (blk.name, n)
        # an output-limited call, then the rest: the state is carried
        blk2, cap = make(), max(1, n // 3)
        st, c, p, need, y1 = blk2.work(src[:n], cap)
        assert (st, c, p, need) == sync_rule(n, cap)
        y2 = blk2.work(src[c:n], n)[4] if c < n else y1[:0]
        assert np.array_equal(np.concatenate([y1, y2]), want[:n]), (blk2.name, n)
    cac = rr.CorrelateAccessCodeTag(HDLC_FLAG, 1)
    check_sync_counts(cac, s["b"][:n])
    assert np.array_equal(run_whole(cac, s["b"][:n]), s["b"][:n])                         # the data passes through
    assert tag_pairs(cac) == [t for t in s["tags"] if t[0] < n]


def test_slicer_special_values():
    f = np.finfo(np.float32)
    vals = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, f.smallest_subnormal, f.tiny, -f.tiny, f.max, -f.max],
                    np.float32)
    x = np.tile(vals, 40)                                 # 520 samples: the 16-byte path and the guarded tail
    want = np.tile(np.array([0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0], np.uint8), 40)
    assert np.array_equal(slicer(x), want)
    assert np.array_equal(run_whole(rr.BinarySlicer(), x), want)
    assert np.array_equal(run_whole(rr.BinarySlicer(), x[:13]), want[:13])


# ---- 2. carried state: any split of the stream gives the one-call output and tags ---------------------------------------------------
_AX = {}


def ax():
    """(x, planted, model bits, model tags) of 30 frames, ~ 5 T samples"""
    if not _AX:
        x, planted = ax25ish_symbols(30, 9)
        bits, pos, diffs = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG).run(x)
        assert 3 * T + 17 < len(x) < 8 * T
        _AX.update(x=x, planted=planted, bits=bits, tags=list(zip(pos.tolist(), diffs.tolist())))
        x.setflags(write=False)
    return _AX["x"], _AX["planted"], _AX["bits"], _AX["tags"]


def feed(blk, x, windows, tagged=True):
    """windows = [(in_len, out_cap)]: every call's counts must be the sync rule's -> (concatenated output, stream-relative tags
    of a block with a correlator stage)"""
    pos, outs, tags = 0, [], []
    for in_len, out_cap in windows:
        in_len = min(in_len, len(x) - pos)
        st, c, p, need, y = blk.work(x[pos:pos + in_len], out_cap)
        assert (st, c, p, need) == sync_rule(in_len, out_cap), (pos, in_len, out_cap)
        if tagged and hasattr(blk, "tags"):
            t = tag_pairs(blk)
            assert all(q < p for q, _ in t)
            tags += [(pos + q, d) for q, d in t]
        outs.append(y); pos += c
    assert pos == len(x)
    return np.concatenate(outs), tags


def cut_windows(n, cuts, seed):
    """windows that end exactly at every cut; between cuts random lengths of 1 .. 2 T, some output-limited; (0, 100) and (w, 0)
    calls in between"""
    rng = np.random.default_rng(seed)
    windows, pos = [], 0
    for c in sorted(set(cuts)) + [n]:
        while pos < c:
            w = min(int(rng.integers(1, 2 * T + 1)), c - pos)
            cap = int(rng.integers(1, w + 1)) if rng.random() < 0.3 else w
            if len(windows) % 4 == 1:
                windows += [(0, 100), (w, 0)]
            windows.append((w + int(rng.integers(0, 50)), cap) if cap < w else (w, cap)); pos += min(w, cap)
    return windows


def test_carried_state_any_split():
    x, planted, bits, tags = ax()
    n = len(x)
    one = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    y, t = feed(one, x, [(n, n)])
    assert np.array_equal(y, bits) and t == tags
    assert set(planted.tolist()) <= {p for p, d in t if d == 0}
    p1 = int(planted[planted > 2 * T][0])                 # a flag's last bit: cuts inside the sync word ...
    p2 = int(planted[planted > 3 * T][2])
    cuts = [5, 5 + 40,                                    # a short window at the start of the stream, then 40 one-sample calls
            p1 - 3, p1 - 2, p2, p2 + 9,                   # inside a sync word; inside the 17 bits the descrambler reaches back
            T + 1, 2 * T + 1, 2 * T + 1 + 100,            # one sample after a tile boundary; fewer than 128 samples after a long window
            3 * T, 3 * T + 127]
    w = [(5, 5)] + [(1, 1)] * 40 + cut_windows(n - 45, [c - 45 for c in cuts[2:]], 4)
    assert (0, 100) in w and any(cap < ln for ln, cap in w if cap)
    y2, t2 = feed(rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG), x, w)
    assert np.array_equal(y2, bits) and t2 == tags
    # a window of fewer than 128 samples right behind a long one, spelled out: 2 T + 3, then 100, 1, 127, 64, then the rest;
    # and the same behind a window that ends one sample after a tile boundary of its own
    w = [(2 * T + 3, 2 * T + 3), (100, 100), (1, 1), (127, 127), (64, 64), (T + 1, T + 1), (17, 17), (n, n)]
    assert sum(a for a, _ in w[:-1]) < n
    y2, t2 = feed(rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG), x, w)
    assert np.array_equal(y2, bits) and t2 == tags
    # every stage's carry alone: the four single blocks chained through host arrays, every one on its own random split
    a, _ = feed(rr.BinarySlicer(), x, cut_windows(n, cuts, 5))
    b, _ = feed(rr.NrziDecode(), a, cut_windows(n, cuts, 6))
    c, _ = feed(rr.Descrambler.g3ruh(), b, cut_windows(n, cuts, 7))
    d, t3 = feed(rr.CorrelateAccessCodeTag(HDLC_FLAG, 0), c, cut_windows(n, cuts, 8))
    assert np.array_equal(a, slicer(x)) and np.array_equal(c, bits) and np.array_equal(d, bits) and t3 == tags


def test_a_call_that_moves_nothing_keeps_the_state_and_has_no_tags():
    blk = rr.CorrelateAccessCodeTag([1, 0], 0)
    assert blk.work(np.array([1], np.uint8), 1)[4].tolist() == [1] and tag_pairs(blk) == []
    assert blk.work(np.array([0], np.uint8), 0)[2] == 0 and tag_pairs(blk) == []
    assert blk.work(np.array([0], np.uint8), 1)[4].tolist() == [0] and tag_pairs(blk) == [(0, 0)]      # the 1 before it is remembered


def test_more_tiles_than_workgroups():
    """the kernel launches at most 8 workgroups per compute unit and strides them over the tiles: a window of 12 tiles per compute
    unit gives every workgroup one or two tiles, the arrays in LDS are used again, and the tag list has thousands of tile
    regions to gather.  Against the vectorised model (tests/test_bits_cpu.py holds that to the state machines); the flag with
    2 differences allowed tags about one position in seven."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (12 * cus + 3) * T + 17
    x = np.random.default_rng(31).normal(0.0, 1.0, n).astype(np.float32)
    want_bits, want_pos, want_diffs = chain_vectorised(x, HDLC_FLAG, 2)
    assert len(want_pos) > n // 10
    blk = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG, allowed_diffs=2)
    assert np.array_equal(run_whole(blk, x), want_bits)
    pos, diffs = blk.tags()
    assert np.array_equal(pos, want_pos) and np.array_equal(diffs, want_diffs)
    # the carried state after such a window: a short one behind it
    m = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG, allowed_diffs=2)
    m.nrzi.last = int(slicer(x[-1:])[0])
    m.lfsr.shift_reg = sum(int(b) << (16 - k) for k, b in enumerate((np.uint8(1) ^ slicer(x[-18:])[1:] ^ slicer(x[-18:])[:-1])[::-1]))
    m.slide.slide = want_bits[-8:].tolist()
    tail = x[1000:1100]
    wb, wp, wd = m.run(tail)
    assert np.array_equal(run_whole(blk, tail), wb)
    pos, diffs = blk.tags()
    assert np.array_equal(pos, wp) and np.array_equal(diffs, wd)


# ---- 3. descrambler parameters -------------------------------------------------------------------------------------------------------
_FULL64 = (1 << 64) - 1


@pytest.mark.parametrize("mask,seed,length", [
    G3RUH, (1, 0, 0), (1, 1, 0), (0, 0, 0), (3, 2, 1), (1, 3, 1), (0x21, 0x1ABCD, 16), (1 << 16, 1, 16), ((1 << 17) - 1, 0x15555, 16),
    (1, 1 << 63, 63), (1 << 63, 1, 63), (_FULL64, 0xDEADBEEFCAFEF00D, 63), (0x8000000000000001, 5, 63),
    (0x21 | 0xABC << 17, 0, 16), (1 | 6 << 1, 1, 0)],
    ids=["g3ruh", "len0", "len0-seed", "mask0", "len1-all", "len1-one", "g3ruh-seed", "len16-top-bit", "len16-all", "len63-bit0",
         "len63-bit63", "len63-all", "len63-ends", "bits-above-len", "len0-bits-above"])
def test_descrambler_parameters(mask, seed, length):
    b = shared()["b"][:2 * T + 77]
    want = np.array(Lfsr(mask, seed, length).run(b), np.uint8)
    got = run_whole(rr.Descrambler(mask, seed, length), b)
    assert np.array_equal(got, want)
    if seed:                                                # output k < len + 1 sees the seed through parity((seed >> k) & mask)
        low = mask & ((2 << length) - 1)
        shows = any(bin((seed >> k) & low).count("1") & 1 for k in range(length + 1))
        zero = np.array(Lfsr(mask, 0, length).run(b[:length + 1]), np.uint8)
        assert (not np.array_equal(zero, want[:length + 1])) == shows
        assert np.array_equal(np.array(Lfsr(mask, 0, length).run(b), np.uint8)[length + 1:], want[length + 1:])
    if mask >> (length + 1):
        assert np.array_equal(want, np.array(Lfsr(mask & ((2 << length) - 1), seed, length).run(b), np.uint8))
    # the same in the fused block behind the slicer, split in three
    x = (2.0 * b.astype(np.float32) - 1.0)
    fused = rr.BitDecoder(descrambler=(mask, seed, length))
    y, _ = feed(fused, x, [(100, 100), (T, T), (len(x), len(x))], tagged=False)
    assert np.array_equal(y, want)


# ---- 4. the correlator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 8, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("allowed", [0, 3, "L"])
def test_correlator_lengths(L, allowed):
    rng = np.random.default_rng(100 + L)
    code = rng.integers(0, 2, L).tolist()
    allowed = L + 5 if allowed == "L" else allowed
    n = T + 300
    b = rng.integers(0, 2, n).astype(np.uint8)
    b[:L] = code                                            # a match ending at sample L - 1 of the stream, the first possible
    b[T - L // 2:T - L // 2 + L] = code                     # a code that straddles two tiles
    b[T + 100:T + 100 + L] = code                           # ... and one that straddles two calls (below)
    b[T + 200:T + 200 + L] = code
    b[T + 200 + L // 2] ^= 1                                # one difference
    want = Slide(code, allowed).run(b)
    assert (L - 1, 0) in want and all(p >= L - 1 for p, _ in want)
    blk = rr.CorrelateAccessCodeTag(code, allowed)
    assert np.array_equal(run_whole(blk, b), b)
    got = tag_pairs(blk)
    assert got == want
    if allowed >= L:                                        # every position from L - 1 on, and none before
        assert [p for p, _ in got] == list(range(L - 1, n))
    cut = T + 100 + (L + 1) // 2
    y, t = feed(rr.CorrelateAccessCodeTag(code, allowed), b, [(cut, cut), (n, n)])
    assert np.array_equal(y, b) and t == want
    if L > 1:                                               # the stream's first L - 1 bits alone: nothing, whatever is allowed
        first = rr.CorrelateAccessCodeTag(code, allowed)
        first.work(b[:L - 1], L - 1)
        assert tag_pairs(first) == []


def test_no_match_and_tag_retrieval():
    blk = rr.CorrelateAccessCodeTag([1] * 8, 0)
    zeros = np.zeros(3 * T + 5, np.uint8)
    run_whole(blk, zeros)
    total = C.c_size_t(99)
    assert rr.lib().rr_bit_tags(blk._h, None, None, 0, C.byref(total)) == 0 and total.value == 0
    b = zeros.copy()
    for p in (10, 2000, T + 1, 3 * T):
        b[p - 7:p + 1] = 1
    run_whole(blk, b)
    assert tag_pairs(blk) == [(10, 0), (2000, 0), (T + 1, 0), (3 * T, 0)]
    pos, diffs = np.full(4, 77, np.uint64), np.full(4, 77, np.uint8)
    assert rr.lib().rr_bit_tags(blk._h, pos.ctypes.data_as(C.c_void_p), diffs.ctypes.data_as(C.c_void_p), 2, C.byref(total)) == 0
    assert total.value == 4 and pos.tolist() == [10, 2000, 77, 77] and diffs.tolist() == [0, 0, 77, 77]     # cap < total
    assert tag_pairs(blk) == [(10, 0), (2000, 0), (T + 1, 0), (3 * T, 0)]                                     # asking twice is fine
    assert rr.lib().rr_bit_tags(rr.BinarySlicer()._h, None, None, 0, C.byref(total)) == rr.ERR
    assert "correlator" in rr.last_error()


# ---- 5. fused against unfused against the model ---------------------------------------------------------------------------------------
def chain_unfused(x, invert, nrzi, descrambler, code, allowed):
    b = run_whole(rr.BinarySlicer(), x)
    if invert:
        b = b ^ np.uint8(1)                                 # XorConst(1), a host step: the library has no such block of its own
    if nrzi:
        b = run_whole(rr.NrziDecode(), b)
    if descrambler is not None:
        b = run_whole(rr.Descrambler(*descrambler), b)
    cac = rr.CorrelateAccessCodeTag(code, allowed)
    b = run_whole(cac, b)
    return b, tag_pairs(cac)


def test_fused_equals_unfused_equals_model_ax25():
    x, planted, bits, tags = ax()
    fused = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    yf = run_whole(fused, x)
    tf = tag_pairs(fused)
    yu, tu = chain_unfused(x, False, True, G3RUH, HDLC_FLAG, 0)
    assert np.array_equal(yf, yu) and tf == tu
    assert np.array_equal(yf, bits) and tf == tags
    assert set(planted.tolist()) <= {p for p, _ in tf} and len(planted) == 60


def test_il2p_configuration():
    """examples/il2p-1200-rx.rs:118-126: BinarySlicer -> XorConst(1) -> CorrelateAccessCodeTag, here a 32-bit code, 1 diff allowed"""
    rng = np.random.default_rng(21)
    b = rng.integers(0, 2, 2 * T + 500).astype(np.uint8)
    for p, flip in ((300, None), (T - 10, 7), (T + 900, None), (2 * T + 100, 31)):
        b[p:p + 32] = IL2P_SYNC32
        if flip is not None:
            b[p + flip] ^= 1
    x = ((1.0 - 2.0 * b) * rng.uniform(0.3, 1.5, len(b))).astype(np.float32)        # inverted on the air
    want_bits, pos, diffs = Chain(invert=True, code=IL2P_SYNC32, allowed_diffs=1).run(x)
    want = list(zip(pos.tolist(), diffs.tolist()))
    assert np.array_equal(want_bits, b) and {(331, 0), (T + 21, 1), (T + 931, 0), (2 * T + 131, 1)} <= set(want)
    fused = rr.BitDecoder(invert=True, code=IL2P_SYNC32, allowed_diffs=1)
    assert np.array_equal(run_whole(fused, x), b) and tag_pairs(fused) == want
    yu, tu = chain_unfused(x, True, False, None, IL2P_SYNC32, 1)
    assert np.array_equal(yu, b) and tu == want


@pytest.mark.parametrize("n", [1, 17, 129, T + 1, 3 * T + 17])
def test_fused_lengths(n):
    x, _, bits, tags = ax()
    blk = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    check_sync_counts(blk, x[:n])
    assert np.array_equal(run_whole(blk, x[:n]), bits[:n])
    assert tag_pairs(blk) == [t for t in tags if t[0] < n]
    assert blk.name == "BitDecoder"


# ---- 6. device windows at odd byte offsets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 3), (5, 0), (0, 7), (16, 16), (3, 3)])
def test_device_windows_unaligned_u8(in_off, out_off):
    import torch
    s = shared()
    n = 2 * T + 333
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + n] = torch.from_numpy(s["b"][:n].copy()).cuda()
    blk = rr.Descrambler.g3ruh()
    assert (d_in.data_ptr() + in_off) % 16 == in_off % 16
    # two calls: the second starts at an odd offset of its own
    first = 1001
    torch.cuda.synchronize()
    assert blk.work_dev(d_in.data_ptr() + in_off, first, d_out.data_ptr() + out_off, first) == sync_rule(first, first)
    assert blk.work_dev(d_in.data_ptr() + in_off + first, n - first, d_out.data_ptr() + out_off + first, n - first) == sync_rule(n - first, n - first)
    blk.sync()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[out_off:out_off + n], s["descr"][:n])
    assert np.all(got[:out_off] == 9) and np.all(got[out_off + n:] == 9)               # nothing outside the window is written


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (1, 5), (2, 16), (4, 1)])
def test_device_windows_f32_input_offset(in_off, out_off):
    import torch
    x, _, bits, tags = ax()
    n = 2 * T + 99
    d_in = torch.zeros(n + 16, dtype=torch.float32, device="cuda")
    d_out = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
    d_in[in_off:in_off + n] = torch.from_numpy(x[:n].copy()).cuda()
    blk = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    torch.cuda.synchronize()
    assert blk.work_dev(d_in.data_ptr() + 4 * in_off, n, d_out.data_ptr() + out_off, n) == sync_rule(n, n)
    assert tag_pairs(blk) == [t for t in tags if t[0] < n]                              # (waits for the call)
    got = d_out.cpu().numpy()
    assert np.array_equal(got[out_off:out_off + n], bits[:n])
    assert np.all(got[:out_off] == 9) and np.all(got[out_off + n:] == 9)


# ---- 7. names, sizes, tag rules ----------------------------------------------------------------------------------------------------------
def test_names_sizes_and_tag_rules():
    p = C.c_size_t(0)
    for blk, name, ies in ((rr.BinarySlicer(), "BinarySlicer", 4), (rr.NrziDecode(), "NrziDecode", 1), (rr.Descrambler.g3ruh(), "Descrambler", 1),
                           (rr.CorrelateAccessCodeTag(HDLC_FLAG), "CorrelateAccessCodeTag", 1), (rr.BitDecoder(nrzi=True), "BitDecoder", 4)):
        assert blk.name == name
        assert rr.lib().rr_block_in_elem_size(blk._h) == ies and rr.lib().rr_block_out_elem_size(blk._h) == 1
        assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == 1 and p.value == 1     # RR_TAGS_FORWARD, position for position
    assert rr.lib().rr_abi_version() == 3


def test_one_launch_per_call():
    x, _, _, _ = ax()
    blk = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    import torch
    d_in = torch.from_numpy(x.copy()).cuda()
    d_out = torch.empty(len(x), dtype=torch.uint8, device="cuda")
    for n in (len(x), 100, 1):
        l0 = int(rr.lib().rr_debug_kernel_launches())
        assert blk.work_dev(d_in.data_ptr(), n, d_out.data_ptr(), n)[2] == n
        assert int(rr.lib().rr_debug_kernel_launches()) - l0 == 1
    blk.sync()


# ---- 8. the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_bits(tmp_path):
    x, planted = ax25ish_symbols(3, 12)
    bits, pos, diffs = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG).run(x)
    assert set(planted.tolist()) <= set(pos.tolist())
    vec = tmp_path / "vectors.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<Q", len(x))); f.write(x.astype("<f4").tobytes()); f.write(bits.tobytes())
        f.write(struct.pack("<Q", len(pos))); f.write(pos.astype("<u8").tobytes()); f.write(diffs.tobytes())
    exe = os.path.join(ROOT, "tests", "cpp", "test_bits_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_bits_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    out = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK")
