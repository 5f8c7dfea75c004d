"""GPU: BurstSaver and Delay of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_saver.hip) on one
short stream, window by window: tests/cpp/test_saver_host.cpp."""
import os
import struct
import subprocess

import numpy as np
import pytest

import burst_model as bm
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_burst_saver_and_delay(tmp_path):
    alpha, thr, delay, max_size, tail = 0.1, 0.004, 300, 2500, 40
    n = 9000
    x = bm.burst_signal(n, 61)
    cuts = [0, 100, 101, 2500, 2500, 5000, n]
    b = rr.BurstSaver(alpha, thr, delay, max_size, tail)
    vec = tmp_path / "vectors.bin"
    npdus = 0
    with open(vec, "wb") as f:
        f.write(struct.pack("<ffQQQQ", alpha, thr, delay, max_size, tail, n))
        f.write(x.astype("<c8").tobytes())
        f.write(struct.pack("<Q", len(cuts) - 1))
        for a, c in zip(cuts[:-1], cuts[1:]):
            rec = b.push(x[a:c])
            f.write(struct.pack("<QQ", c - a, len(rec)))
            for i, r in enumerate(rec):
                p = b.pdu(i, rec)
                f.write(struct.pack("<QQ", int(r["stream_pos"]), len(p))); f.write(p.astype("<c8").tobytes())
                npdus += 1
    assert npdus == 3
    exe = os.path.join(ROOT, "tests", "cpp", "test_saver_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_saver_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
