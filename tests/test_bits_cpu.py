"""CPU-only: the model the GPU tests of the bit-level blocks rely on (tests/bits_model.py) — the reference's own test vectors
through it, the kernel's unrolled descrambler formula against the sequential register, the planted flags of the test signal —
and the public surface of rr_binary_slicer / rr_nrzi_decode / rr_descrambler / rr_correlate_access_code_tag / rr_bit_decoder."""
import ctypes

import numpy as np
import pytest

import rustradio_amd as rr
from bits_model import (G3RUH, HDLC_FLAG, Chain, Lfsr, Nrzi, Slide, ax25ish_symbols, chain_vectorised, descramble_unrolled, hdlc_stuff,
                        nrzi_encode, scramble, slicer)


def test_reference_nrzi_vectors():
    """nrzi.rs tests `encode` (which runs NrziDecode) and `decode` (which runs NrziEncode)"""
    assert Nrzi().run([0, 0, 0, 0, 1, 1, 1, 1]) == [1, 1, 1, 1, 0, 1, 1, 1]
    assert nrzi_encode([1, 1, 1, 1, 0, 1, 1, 1]) == [0, 0, 0, 0, 1, 1, 1, 1]
    # the state is carried: two calls equal one
    n = Nrzi()
    assert n.run([0, 0, 0]) + n.run([0, 1, 1, 1, 1]) == [1, 1, 1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("inp,expect", [
    ([1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0], [1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 0, 0, 1]),
    ([1] * 24, [1] * 12 + [0] * 5 + [1] * 7)], ids=["known_good_test1", "known_good_ones"])
def test_reference_descrambler_vectors(inp, expect):
    scrambled = scramble(inp + [0] * 17)[17:]
    assert scrambled != inp and scrambled == expect
    assert Lfsr(*G3RUH).run(scrambled + [0] * 16)[:len(inp)] == inp
    assert descramble_unrolled(scrambled, *G3RUH) == Lfsr(*G3RUH).run(scrambled)


def test_reference_long_random_nrzi_g3ruh():
    """descrambler.rs long_random_nrzi_g3ruh, seeded: NrziEncode -> Scrambler -> Descrambler -> NrziDecode, 17 bits late"""
    rng = np.random.default_rng(11)
    inp = rng.integers(0, 2, 2000).tolist()
    pad = rng.integers(0, 2, 17).tolist()
    out = Nrzi().run(Lfsr(*G3RUH).run(scramble(nrzi_encode(inp + pad))))
    assert out[17:] == inp


def test_reference_tagged_waits_for_full_code_before_match():
    assert Slide([0, 1], 0).run([1]) == []
    with pytest.raises(AssertionError, match="access code must be nonempty"):
        Slide([], 0)
    s = Slide([0, 1], 0)
    assert s.run([0]) == [] and s.run([1, 0, 1]) == [(0, 0), (2, 0)]           # a code that straddles two calls


def test_slicer_special_values():
    tiny = np.float32(1e-45)
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], np.float32)
    assert slicer(x).tolist() == [0, 1, 0, 0, 0, 1, 0, 1, 0]


def test_unrolled_descrambler_equals_the_register():
    """stage 4 of the kernel against Lfsr::next_descramble: random (mask, seed, len), len 0 and 63 included; mask
    bits above len change nothing"""
    rng = np.random.default_rng(5)
    lens = [0, 1, 16, 62, 63] + rng.integers(0, 64, 195).tolist()
    for length in lens:
        full = (1 << (length + 1)) - 1
        mask = int(rng.integers(0, 1 << 62)) & full
        seed = int(rng.integers(0, 1 << 62)) & full
        d = rng.integers(0, 2, 300).tolist()
        want = Lfsr(mask, seed, length).run(d)
        assert descramble_unrolled(d, mask, seed, length) == want, (mask, seed, length)
        high = mask | (int(rng.integers(1, 1 << 20)) << (length + 1)) & ((1 << 64) - 1)
        assert Lfsr(high, seed, length).run(d) == want


def test_planted_flags_are_found_where_they_were_planted():
    x, planted = ax25ish_symbols(6, 3)
    assert len(planted) == 12 and x.dtype == np.float32
    bits, pos, diffs = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG, allowed_diffs=0).run(x)
    assert len(bits) == len(x) and set(bits.tolist()) <= {0, 1}
    found = dict(zip(pos.tolist(), diffs.tolist()))
    for p in planted.tolist():
        assert found.get(p) == 0, p
        assert bits[p - 7:p + 1].tolist() == HDLC_FLAG
    # stuffing: no run of six ones inside a payload
    assert "111111" not in "".join(map(str, hdlc_stuff([1] * 40)))
    # the split into calls does not matter to the model either
    c = Chain(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)
    b1, p1, _ = c.run(x[:1001])
    b2, p2, _ = c.run(x[1001:])
    assert np.array_equal(np.concatenate([b1, b2]), bits) and np.array_equal(np.concatenate([p1, p2 + np.uint64(1001)]), pos)


def test_vectorised_chain_equals_the_sequential_one():
    """the model of the multi-million-sample GPU test against the state machines, flag and a 33-bit code with differences"""
    x, _ = ax25ish_symbols(8, 17)
    rng = np.random.default_rng(3)
    for code, allowed in ((HDLC_FLAG, 0), (HDLC_FLAG, 2), (rng.integers(0, 2, 33).tolist(), 12)):
        bits, pos, diffs = Chain(nrzi=True, descrambler=G3RUH, code=code, allowed_diffs=allowed).run(x)
        vb, vp, vd = chain_vectorised(x, code, allowed)
        assert len(pos) > 10
        assert np.array_equal(vb, bits) and np.array_equal(vp, pos) and np.array_equal(vd, diffs)


# ---- the generator of tests/test_gpu_bits_fuzz.py, held to its own conditions ------------------------------------------------------
def test_fuzz_generator_meets_its_conditions():
    from test_gpu_bits_fuzz import (CODE_LENS, DESCRAMBLER_LENS, ONES_FIRST, SEEDS, fuzz_case, moving_calls, nrzi_inverse,
                                    unscramble_inverse)
    assert len(SEEDS) == 48
    d = np.random.default_rng(1).integers(0, 2, 300).tolist()
    assert Lfsr(0x8000000000000001, 5, 63).run(unscramble_inverse(d, 0x8000000000000001, 5, 63)) == d
    assert Nrzi().run(nrzi_inverse(d)) == d
    with_tags = quiet_call = long_hard = short = singles = past_64 = 0
    lens, dlens, alloweds = set(), set(), set()
    for seed in SEEDS:
        c = fuzz_case(seed)
        n, L = c["n"], c["L"]
        assert len(c["x"]) == len(c["bits"]) == n and 1 <= n <= 3 * 4096 + 200
        assert np.array_equal(c["bits"], c["s"])                  # the stream decodes to the bits that were drawn and planted
        assert [p for p, _ in c["tags"]] == sorted({p for p, _ in c["tags"]}) and all(L - 1 <= p < n for p, _ in c["tags"])
        found = dict(c["tags"])
        for start in c["plants"]:                                 # a planted code is a certain match
            assert found.get(start + L - 1, 99) <= min(c["allowed"], L), (seed, start)
        calls = moving_calls(c["windows"], n)
        assert calls[:min(ONES_FIRST, n)] == [(i, i + 1) for i in range(min(ONES_FIRST, n))]
        assert [b for _, b, _, _ in c["dev"]][-1] == n and c["dev"][0][0] == 0
        with_tags += bool(c["tags"])
        quiet_call += any(not any(a <= p < b for p in found) for a, b in calls)
        if L:
            lens.add(L); alloweds.add(min(c["allowed"], 65))
            if c["cut"] is not None and len(c["plants"]) == 3:    # one at the start, one across the tile seam, one across a call cut
                assert c["plants"][0] == 0 and c["plants"][1] <= 4096 < c["plants"][1] + L and c["plants"][2] < c["cut"] <= c["plants"][2] + L
                assert any(b == c["cut"] for _, b in calls)
                past_64 += L > 8
        if c["descrambler"] is not None:
            dlens.add(c["descrambler"][2])
        long_hard += L >= 33 and c["nrzi"] and c["descrambler"] is not None and c["descrambler"][2] == 63 and len(c["plants"]) == 3
        short += 1 <= L <= 32
        singles += c["single"] is not None
    print(f"{with_tags} cases with tags, {quiet_call} with a call without, code lengths {sorted(lens)}, descrambler lengths "
          f"{sorted(dlens)}, allowed {sorted(alloweds)}, {singles} single-stage, {past_64} with L > 8 and all three plants")
    assert with_tags >= 12 and quiet_call >= 12 and long_hard >= 1 and short >= 1
    assert lens == set(CODE_LENS) and dlens == set(DESCRAMBLER_LENS) and alloweds >= {0, 1, 3, 65}
    assert singles >= 5 and past_64 >= 5


# ---- public surface ----------------------------------------------------------------------------------------------------------
_U64, _UINT, _SZ = ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_size_t


def _create(name, *args):
    """the raw constructor -> 'ok' | the library's error.  Without a device good parameters still fail, later."""
    h = getattr(rr.lib(), name)(*args)
    if h:
        rr.lib().rr_block_destroy(h)
        return "ok"
    return rr.last_error()


def test_parameter_errors():
    big = (1 << 64) - 1
    assert _create("rr_descrambler_create", 0x21, 0, 64) == "descrambler length out of range"
    assert _create("rr_descrambler_create", 0x21, 1 << 17, 16) == "seed wider than the register"
    assert _create("rr_descrambler_create", 1, 2, 0) == "seed wider than the register"
    assert _create("rr_correlate_access_code_tag_create", 0, 0, 0) == "access code must be nonempty"
    assert _create("rr_correlate_access_code_tag_create", 1, 65, 0) == "access code longer than 64 bits"
    assert _create("rr_bit_decoder_create", 4, 0x21, 0, 64, 0, 0, 0) == "descrambler length out of range"
    assert _create("rr_bit_decoder_create", 4, 0x21, 1 << 17, 16, 0, 0, 0) == "seed wider than the register"
    assert _create("rr_bit_decoder_create", 0, 0, 0, 0, 0, 65, 0) == "access code longer than 64 bits"
    assert _create("rr_bit_decoder_create", 8, 0, 0, 0, 0, 0, 0) == "unknown bit decoder flags"
    for good in (("rr_descrambler_create", 0x21, 0, 16), ("rr_descrambler_create", big, (1 << 63) | 1, 63),
                 ("rr_descrambler_create", 1, 1, 0), ("rr_correlate_access_code_tag_create", big, 64, 1000),
                 ("rr_bit_decoder_create", 7, 0x21, 0, 16, 0x7E, 8, 0), ("rr_bit_decoder_create", 0, 0, 0, 0, 0, 0, 0),
                 ("rr_bit_decoder_create", 3, 1, 1 << 40, 99, 0, 0, 0)):      # (no DESCRAMBLE flag: mask, seed, len are not read)
        msg = _create(*good)
        assert msg == "ok" or "no usable HIP device" in msg, (good, msg)
    with pytest.raises(ValueError, match="descrambler length out of range"):
        rr.Descrambler(0x21, 0, 64)
    with pytest.raises(ValueError, match="seed wider than the register"):
        rr.Descrambler(0x21, 1 << 17, 16)
    with pytest.raises(ValueError, match="access code must be nonempty"):
        rr.CorrelateAccessCodeTag([], 0)
    with pytest.raises(ValueError, match="access code longer than 64 bits"):
        rr.CorrelateAccessCodeTag([1] * 65, 0)
    with pytest.raises(ValueError, match="descrambler length out of range"):
        rr.BitDecoder(descrambler=(0x21, 0, 64))
    with pytest.raises(ValueError, match="seed wider than the register"):
        rr.BitDecoder(nrzi=True, descrambler=(0x21, 1 << 17, 16), code=HDLC_FLAG)
    with pytest.raises(ValueError, match="access code longer than 64 bits"):
        rr.BitDecoder(code=[0] * 65)
    with pytest.raises(ValueError, match="access code bits must be 0 or 1"):
        rr.CorrelateAccessCodeTag([0, 2], 0)


def test_public_surface():
    from rustradio_amd._lib import SYMBOLS
    L = rr.lib()
    for s in ("rr_binary_slicer_create", "rr_nrzi_decode_create", "rr_descrambler_create", "rr_correlate_access_code_tag_create",
              "rr_bit_decoder_create", "rr_bit_tags"):
        assert s in SYMBOLS and hasattr(ctypes.CDLL(rr.LIB_PATH), s)
    assert L.rr_descrambler_create.argtypes == [_U64, _U64, _UINT]
    assert L.rr_correlate_access_code_tag_create.argtypes == [_U64, _UINT, _SZ]
    assert L.rr_bit_decoder_create.argtypes == [ctypes.c_int, _U64, _U64, _UINT, _U64, _UINT, _SZ]
    assert (rr.BITS_INVERT, rr.BITS_NRZI, rr.BITS_DESCRAMBLE) == (1, 2, 4)
    assert rr.pack_code(HDLC_FLAG) == (0x7E, 8) and rr.pack_code([1, 0, 0]) == (1, 3)      # code[0], the oldest bit, in bit 0
    assert callable(rr.BinarySlicer) and callable(rr.NrziDecode) and callable(rr.Descrambler.g3ruh)
    assert callable(rr.CorrelateAccessCodeTag.tags) and callable(rr.BitDecoder.tags)
    assert L.rr_abi_version() == 3
    total = ctypes.c_size_t(7)
    assert L.rr_bit_tags(None, None, None, 0, ctypes.byref(total)) == rr.ERR           # no handle: an error, never a crash
    makes = {"BinarySlicer": rr.BinarySlicer, "NrziDecode": rr.NrziDecode, "Descrambler": rr.Descrambler.g3ruh,
             "CorrelateAccessCodeTag": lambda: rr.CorrelateAccessCodeTag(HDLC_FLAG, 0),
             "BitDecoder": lambda: rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=HDLC_FLAG)}
    import torch
    if not torch.cuda.is_available():            # no CPU fallback: constructing any of them needs a device
        for make in makes.values():
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
        return
    for name, make in makes.items():             # with a device: names, element sizes, the tag rule, rr_bit_tags on a slicer
        b = make()
        assert b.name == name
        param = ctypes.c_size_t(0)
        assert L.rr_block_tag_rule(b._h, ctypes.byref(param)) == 1 and param.value == 1       # RR_TAGS_FORWARD
        rc = L.rr_bit_tags(b._h, None, None, 0, ctypes.byref(total))
        assert rc == (0 if name in ("CorrelateAccessCodeTag", "BitDecoder") else rr.ERR), name
    assert L.rr_bit_tags(rr.BitDecoder(nrzi=True)._h, None, None, 0, ctypes.byref(total)) == rr.ERR    # code_len 0: no correlator
