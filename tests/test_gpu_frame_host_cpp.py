"""GPU: the transmit chain of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_frame.hip, kernels_tx.hip):
tests/cpp/test_frame_host.cpp frames the packets written here and modulates the levels; its levels must be the sequential
model's bit for bit, and its Complex stream the long-double truth of tests/tx_model.py fed where(bits, hi, lo), within the
bound tests/tx_model.py derives for rr_fm_tx."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import frame_model as fm
from tx_model import bound, comp_err, fm_tx_truth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_framer_into_fm_tx(tmp_path):
    rng = np.random.default_rng(61)
    packets = fm.draw_packets(rng, 12, 90)
    interp, deci, lo, hi = 5, 1, -1.0, 1.0
    k = 2.0 * math.pi * 3000.0 / 48000.0                    # |k a| <= 2 pi: the range of tx_model.bound
    vec, out = tmp_path / "packets.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<QQdffQ", interp, deci, k, lo, hi, len(packets)))
        for p in packets:
            f.write(struct.pack("<Q", len(p))); f.write(p)
    exe = os.path.join(ROOT, "tests", "cpp", "test_frame_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_frame_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw = open(out, "rb").read()
    nl = struct.unpack_from("<Q", raw, 0)[0]
    levels = np.frombuffer(raw, "<f4", nl, 8)
    nc = struct.unpack_from("<Q", raw, 8 + 4 * nl)[0]
    y = np.frombuffer(raw, "<c8", nc, 16 + 4 * nl)
    bits = fm.FramerSeq(fm.FCS | fm.G3RUH | fm.NRZI).push(packets)[0]
    want = np.where(bits != 0, np.float32(hi), np.float32(lo))
    assert nl == len(want) and np.array_equal(levels, want)
    assert nc == nl * interp // deci
    e = comp_err(y, fm_tx_truth(want, interp, deci, k, nc))
    print(f"{nc} outputs, worst component error {e:.4e}, bound {bound(nc):.4e}")
    assert e <= bound(nc)
