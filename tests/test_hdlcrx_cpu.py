"""No GPU: the ABI surface of rr_hdlc_receiver, its host-only logic (rustradio_amd/csrc/hdlcrx_host.hpp) as a stand-alone program
under the host sanitizers, its word-form bit chain (rustradio_amd/csrc/hdlcrx_core.hpp) run thread by thread under g++ against the
bit-serial NrziDecode / Lfsr, and the end-to-end condition the SymbolSync -> HdlcReceiver test of tests/test_gpu_hdlcrx.py relies
on, asserted on the models."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hdlcrx_helpers as hx
import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rr_hdlc_receiver_create", "rr_hdlc_receiver_push_dev", "rr_hdlc_receiver_push", "rr_hdlc_receiver_frames",
               "rr_hdlc_receiver_frame_bytes", "rr_hdlc_receiver_bytes_dev", "rr_hdlc_receiver_stats", "rr_hdlc_receiver_consumed",
               "rr_hdlc_receiver_dims")


def _build(src, exe, extra):
    subprocess.run(["g++", "-std=c++17", *extra, src, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_abi_surface(tmp_path):
    """every new symbol is declared in the header, exported by the library, listed and typed in _lib.py; rr_hdlc_stream_frame is 32
    bytes in C and in numpy; RR_ABI_VERSION stays 3"""
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
    sz, u64, vp, psz = ctypes.c_size_t, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)
    assert typed.rr_hdlc_receiver_create.argtypes == [sz, ctypes.c_int, u64, u64, ctypes.c_uint, sz, sz, ctypes.c_int]
    assert typed.rr_hdlc_receiver_push_dev.argtypes == [vp, vp, sz, sz, vp, vp]
    assert typed.rr_hdlc_receiver_stats.argtypes == [vp, vp, vp, vp, sz, psz]
    assert re.search(r"#define\s+RR_ABI_VERSION\s+3\b", header) and typed.rr_abi_version() == 3
    f = rr.HDLC_STREAM_FRAME.fields
    assert rr.HDLC_STREAM_FRAME.itemsize == 32
    assert [f[k][1] for k in ("pos", "start", "len", "flags", "stream", "reserved")] == [0, 8, 16, 20, 24, 28]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "rustradio_amd.h"\n'
                   "_Static_assert(sizeof(rr_hdlc_stream_frame) == 32, \"size\");\n"
                   "_Static_assert(offsetof(rr_hdlc_stream_frame, stream) == 24, \"stream\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """every refusal, the bounds, the clamping of counts and positions, the validation fed hostile device output (another stream's
    arena region, stream == nstreams, a duplicate pos within a stream and the same pos in two, a counter that ran backwards) and
    the copy-outs, as a stand-alone program built with -fsanitize=address,undefined"""
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    out = _build(os.path.join(ROOT, "tests", "cpp", "test_hdlcrx_hostlogic.cpp"), str(tmp_path / "test_hdlcrx_hostlogic"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("hdlcrx host logic ok")


def test_word_form_bit_chain_on_the_cpu(tmp_path):
    """the mark stage's bit chain, thread by thread, against the bit-serial machines: G3RUH, a delay of 64, a non-zero seed, every
    RR_BITS_* combination; lengths 0, 1, 63, 64, 65, 4,097, whole and cut in two at every point up to 130"""
    out = _build(os.path.join(ROOT, "tests", "cpp", "emu_hdlcrx.cpp"), str(tmp_path / "emu_hdlcrx"),
                 ["-O2", "-I", os.path.join(ROOT, "rustradio_amd", "csrc")])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("hdlcrx core ok")


def test_refusals_come_before_any_device():
    for args, msg in (((0, 1, 10), "nstreams out of range"), ((4097, 1, 10), "nstreams out of range"),
                      ((2, 1, 65536), "hdlc deframer: max_size beyond 65535")):
        with pytest.raises(ValueError, match=msg):
            rr.HdlcReceiver(*args)
    with pytest.raises(ValueError, match="unknown hdlc deframer flags"):
        rr.HdlcReceiver(2, 1, 10, flags=4)
    with pytest.raises(ValueError, match="descrambler length out of range"):
        rr.HdlcReceiver(2, 1, 10, descrambler=(0x21, 0, 64))
    with pytest.raises(ValueError, match="seed wider than the register"):
        rr.HdlcReceiver(2, 1, 10, descrambler=(0x21, 1 << 17, 16))
    L = rr.lib()
    assert L.rr_hdlc_receiver_create(2, 8, 0, 0, 0, 1, 10, 0) is None and rr.last_error() == "unknown bit decoder flags"
    assert L.rr_hdlc_receiver_create(0, 8, 0, 0, 0, 1, 10, 4) is None and rr.last_error() == "nstreams out of range"


def test_the_models_deliver_every_frame_of_the_chain_test():
    """the condition the SymbolSync -> HdlcReceiver GPU test relies on: with sps 4.0, max_deviation 0 and hold offset 0 the models
    deliver 3 of 3 frames in every stream, whole and in two pushes cut mid-frame"""
    x = hx.chain_samples()
    assert x.shape[0] == hx.CHAIN_N
    n = x.shape[1]
    for cuts in ([n], [hx.CHAIN_CUT, n - hx.CHAIN_CUT]):
        syms, frames, stats = hx.chain_model(x, cuts)
        for c in range(hx.CHAIN_N):
            got = [f[1] for push in frames for f in push[c]]
            assert got == hx.chain_payloads(c), (cuts, c)
            assert stats[c] == (3, 0, 0)
    # the cut lies inside the first frame of every stream: behind its opening flags (20 + 2 + c of them, 17 bits late behind the
    # scrambler) and in front of its closing flag
    for c in range(hx.CHAIN_N):
        at = len(syms[0][c])
        assert 8 * (22 + c) + 17 < at < frames[1][c][0][0] and frames[0][c] == []
