"""No GPU: the yardstick of rr_il2p_receiver (tests/il2p_model.py) on the reference's own test vector, the ABI surface, the
arithmetic of rustradio_amd/csrc/il2p_core.hpp run thread by thread under g++ against bit-serial code, the host-only logic
(rustradio_amd/csrc/il2p_host.hpp) as a stand-alone program under the host sanitizers, the refusals that come before any device,
and the conditions the GPU tests of tests/test_gpu_il2p.py rely on, asserted on the models."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import il2p_cases as ic
import il2p_model as im
import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rr_il2p_receiver_create", "rr_il2p_receiver_push_dev", "rr_il2p_receiver_push", "rr_il2p_receiver_headers",
               "rr_il2p_receiver_stats", "rr_il2p_receiver_consumed", "rr_il2p_receiver_dims")
OFFSETS = dict(pos=0, stream=8, payload_size=12, pid=14, control=15, flags=16, diffs=17, dst_ssid=18, src_ssid=19, raw=20, dst=35,
               src=42, reserved=49)


def _build(src, exe, extra):
    subprocess.run(["g++", "-std=c++17", *extra, src, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_the_model_on_the_golden_bits_whatever_the_windows():
    """testdata/il2p.bits of the reference (il2p_deframer.rs:374-388): exactly one tag, at 785, and one header with the values
    below, whether the state machine gets one window or windows of 1, 23, 24, 120, 121 and 500 bits: the split-independence claim
    on the reference's own state machine"""
    bits = im.golden_bits()
    assert len(bits) == 1177 and set(bits.tolist()) == {0, 1}
    g = im.GOLDEN
    for size in (None, 1, 23, 24, 120, 121, 500):
        headers, tags = im.run(bits, 0, None if size is None else [size] * (len(bits) // size + 1))
        assert tags == [(785, 0)], size
        assert len(headers) == 1, size
        h = headers[0]
        assert {k: h[k] for k in g} == g, size
        assert h["raw"].hex() == "92a5103171712d10346823001154eb"
    assert im.build_header() == g["raw"]                       # the inverse gives the same 15 bytes back
    assert im.decode(im.scramble(g["raw"])) == [(b >> (7 - i)) & 1 for b in g["raw"] for i in range(8)]


def test_abi_surface(tmp_path):
    """every new symbol is declared in the header, exported by the library, listed and typed in _lib.py; rr_il2p_header is 64 bytes
    with the same offsets in C and in numpy; RR_ABI_VERSION stays 3"""
    from rustradio_amd._lib import SYMBOLS
    header = open(os.path.join(ROOT, "include", "rustradio_amd.h")).read()
    exported = ctypes.CDLL(rr.LIB_PATH)
    typed = rr.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in SYMBOLS and hasattr(exported, s), s
        fn = getattr(typed, s)
        assert fn.argtypes is not None and len(fn.argtypes) >= 2, s
        assert fn.restype in (ctypes.c_int, ctypes.c_void_p), s
    sz, vp, psz = ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)
    assert typed.rr_il2p_receiver_create.argtypes == [sz, ctypes.c_int, sz]
    assert typed.rr_il2p_receiver_push_dev.argtypes == [vp, vp, sz, sz, vp, vp]
    assert typed.rr_il2p_receiver_push.argtypes == [vp, vp, sz, sz, psz]
    assert typed.rr_il2p_receiver_stats.argtypes == [vp, vp, vp, sz, psz]
    assert re.search(r"#define\s+RR_ABI_VERSION\s+3\b", header) and typed.rr_abi_version() == 3
    f = rr.IL2P_HEADER.fields
    assert rr.IL2P_HEADER.itemsize == 64
    assert {k: f[k][1] for k in f} == OFFSETS
    assert f["raw"][0].shape == (15,) and f["reserved"][0].shape == (15,) and f["dst"][0].itemsize == 7 and f["src"][0].itemsize == 7
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "rustradio_amd.h"\n'
                   "_Static_assert(sizeof(rr_il2p_header) == 64, \"size\");\n"
                   + "".join("_Static_assert(offsetof(rr_il2p_header, %s) == %d, \"%s\");\n" % (k, v, k) for k, v in OFFSETS.items())
                   + "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)


def test_core_arithmetic_on_the_cpu(tmp_path):
    """il2p_core.hpp as the three kernels use it, thread by thread, against a bit-serial correlator, chain rule, Lfsr and parse:
    match words for allowed_diffs 0, 1, 3 and 24 at lengths 0, 1, 23, 24, 63, 64, 65 and 4,097, whole and cut in two at every point
    up to 150; the descramble on 1,000 random headers; tile maps composed over 1 to 9 tiles for every entry state, sparse, dense,
    and with a match exactly at free_from - 1 and at free_from"""
    out = _build(os.path.join(ROOT, "tests", "cpp", "emu_il2p.cpp"), str(tmp_path / "emu_il2p"),
                 ["-O2", "-I", os.path.join(ROOT, "rustradio_amd", "csrc")])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("il2p core ok")


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """every refusal, the bounds, the clamping of positions, the validation fed hostile device output (stream == nstreams, a pos
    beyond the stream's range of the push, two headers of one stream closer than 121, a count above the list) and the copy-outs, as a
    stand-alone program built with -fsanitize=address,undefined"""
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    out = _build(os.path.join(ROOT, "tests", "cpp", "test_il2p_hostlogic.cpp"), str(tmp_path / "test_il2p_hostlogic"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("il2p host logic ok")


def test_refusals_come_before_any_device():
    for n in (0, 4097):
        with pytest.raises(ValueError, match="nstreams out of range"):
            rr.Il2pReceiver(n)
    for flags in (rr.BITS_NRZI, rr.BITS_DESCRAMBLE, rr.BITS_INVERT | rr.BITS_NRZI, 8, -1):
        with pytest.raises(ValueError, match="il2p receiver: unknown bit flags"):
            rr.Il2pReceiver(2, bit_flags=flags)
    L = rr.lib()
    assert L.rr_il2p_receiver_create(0, 8, 0) is None and rr.last_error() == "nstreams out of range"
    assert L.rr_il2p_receiver_create(3, 2, 1 << 40) is None and rr.last_error() == "il2p receiver: unknown bit flags"


def test_no_fuzz_case_of_the_gpu_test_is_empty():
    """every seed of tests/test_gpu_il2p.py::test_seeded_fuzz yields at least one header and at least one dropped tag, on the model"""
    for seed in ic.FUZZ_SEEDS:
        streams, pushes, allowed, _ = ic.fuzz_case(seed)
        assert 1 <= len(streams) <= 3 and all(len(s) <= 20000 for s in streams) and 0 <= allowed <= 3
        per_push, stats, consumed = ic.expected(streams, pushes, allowed)
        assert consumed == [len(s) for s in streams], seed
        headers, syncs = sum(s[0] for s in stats), sum(s[1] for s in stats)
        assert headers >= 1 and syncs > headers, (seed, stats)
        assert sum(len(p) for p in per_push) == headers


def test_the_loopback_line_carries_its_headers_on_the_models():
    """the condition of tests/test_gpu_il2p.py::test_loopback_through_the_transmitter: the line (preamble, two frames, tail) through
    the models of the same blocks — fsk_model.seq_chain (AFSK, bell202 tones), the float64 AfskDemod, symsync_model.SymbolSync —
    slices to bits in which il2p_model finds both headers, without inversion: rr_fsk_tx sends a 1 as the higher tone, which the
    demodulator's offset of -1700 Hz leaves positive"""
    import afsk_model as am
    import fsk_model as fk
    import symsync_model as sm
    line, sent = ic.loopback_line()
    t = fk.LOOP_TX
    audio, _, _ = fk.seq_chain(fk.AFSK, line, [len(line)], t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], 1, 1, 0.0)
    soft = fk.demod_f64(audio)
    syms = sm.SymbolSync(*am.SYNC_PRM).run(soft)[0]
    headers, _ = im.run((np.asarray(syms) > 0).astype(np.uint8), 0)
    assert [h["raw"] for h in headers] == sent
