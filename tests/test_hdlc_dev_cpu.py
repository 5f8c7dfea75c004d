"""No GPU: the arithmetic of rustradio_amd/csrc/hdlc_core.hpp run thread by thread on the CPU against the reference's sequential
machine, the host-only logic of the fetch path (rustradio_amd/csrc/hdlc_host.hpp) under the host sanitizers, and what
rr.HdlcDeframer says without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(src, exe, extra):
    subprocess.run(["g++", "-std=c++17", *extra, src, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


def test_hdlc_core_on_the_cpu(tmp_path):
    """predicates, gap maps, the resolved chain and the frames for every bit string of up to 20 bits behind every entry state
    (short ones also cut into two pushes at every point); map composition; CRC chunks; the syndrome search against brute-force
    find_right_crc up to 4,200 bytes with a two-hit case; the carry bound; drawn streams in random pushes"""
    out = _build(os.path.join(ROOT, "tests", "cpp", "emu_hdlc.cpp"), str(tmp_path / "emu_hdlc"),
                 ["-O2", "-I", os.path.join(ROOT, "rustradio_amd", "csrc")])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("hdlc core ok")


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """the refusals, the bounds, the validation fed hostile device output and the clamped copy-outs as a stand-alone program built
    with -fsanitize=address,undefined (rustradio_amd/csrc/hdlc_host.hpp compiles without HIP)"""
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    out = _build(os.path.join(ROOT, "tests", "cpp", "test_hdlc_hostlogic.cpp"), str(tmp_path / "test_hdlc_hostlogic"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("hdlc host logic ok")


NEW_SYMBOLS = ("rr_hdlc_deframer_create", "rr_hdlc_deframer_push_dev", "rr_hdlc_deframer_push", "rr_hdlc_frames", "rr_hdlc_frame_bytes",
               "rr_hdlc_bytes_dev", "rr_hdlc_stats", "rr_hdlc_deframer_dims")


def test_symbols_and_record_layout():
    from rustradio_amd._lib import SYMBOLS
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in SYMBOLS and hasattr(L, s)
    f = rr.HDLC_FRAME.fields
    assert rr.HDLC_FRAME.itemsize == 24
    assert (f["pos"][1], f["start"][1], f["len"][1], f["flags"][1]) == (0, 8, 16, 20)
    assert (rr.HDLC_KEEP_CHECKSUM, rr.HDLC_FIX_BITS) == (1, 2)


def test_every_new_symbol_has_explicit_types():
    L = rr._raw_lib() if hasattr(rr, "_raw_lib") else rr.lib()
    for s in NEW_SYMBOLS:
        fn = getattr(L, s)
        assert fn.argtypes is not None and len(fn.argtypes) >= 2, s
        assert fn.restype in (ctypes.c_int, ctypes.c_void_p), s
    assert L.rr_hdlc_stats.argtypes[1:] == [ctypes.POINTER(ctypes.c_ulonglong)] * 3
    assert L.rr_hdlc_deframer_create.argtypes == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    assert L.rr_hdlc_deframer_push_dev.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]


def test_refusals_come_before_any_device():
    with pytest.raises(ValueError, match="unknown hdlc deframer flags"):
        rr.HdlcDeframer(1, 10, 4)
    with pytest.raises(ValueError, match="unknown hdlc deframer flags"):
        rr.HdlcDeframer(1, 10, -1)
    with pytest.raises(ValueError, match="hdlc deframer: max_size beyond 65535"):
        rr.HdlcDeframer(1, 65536, 0)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert rr.HdlcDeframer(0, 0).name == "HdlcDeframer"
    else:
        with pytest.raises(ValueError, match="no usable HIP device"):
            rr.HdlcDeframer(1, 10, rr.HDLC_FIX_BITS)
