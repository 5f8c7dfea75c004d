"""GPU: StreamToPdu of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_pdu.hip) against the
sequential model, window by window: tests/cpp/test_pdu_host.cpp."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pdu_model as pm
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_cpp_mirror_stream_to_pdu(tmp_path):
    rng = np.random.default_rng(51)
    thr, max_size, tail = 0.5, 700, 6
    bursts = [(40, 300), (400, 9), (420, 650), (1400, 1), (1500, 696), (2300, 500)]      # (start, length); the last but one is too long
    n = 3000
    data = np.zeros(n, F32)
    trig = np.zeros(n, F32)
    for s, length in bursts:
        data[s:s + length + tail] = pm.noisy_nrz_burst(rng, length + tail, 5.2, 0.3, 0.1)
        trig[s:s + length] = 1.0
    data[1400:1407] = 2.0                                            # a constant PDU: Midpointer pushes nothing
    cuts = [0, 100, 101, 700, 700, 1503, 2900, n]
    want = pm.stream_to_pdu_seq(data, trig, thr, max_size, tail, cuts[1:-1])
    b = rr.StreamToPdu(thr, max_size, tail, rr.PDU_MIDPOINT)
    vec = tmp_path / "vectors.bin"
    oks = []
    with open(vec, "wb") as f:
        f.write(struct.pack("<fQQQ", thr, max_size, tail, n))
        f.write(data.astype("<f4").tobytes()); f.write(trig.astype("<f4").tobytes())
        f.write(struct.pack("<Q", len(want)))
        for (a, c), w in zip(zip(cuts[:-1], cuts[1:]), want):
            rec = b.push(data[a:c], trig[a:c])
            assert [int(r["stream_pos"]) for r in rec] == [first for first, _ in w]
            f.write(struct.pack("<QQ", c - a, len(w)))
            for r, (first, p) in zip(rec, w):
                f.write(struct.pack("<QQ", first, len(p))); f.write(np.array(p, "<f4").tobytes())
                f.write(struct.pack("<Bf", int(r["ok"]), float(r["mid"])))
                oks.append(int(r["ok"]))
    assert oks == [1, 1, 1, 0, 1], oks
    exe = os.path.join(ROOT, "tests", "cpp", "test_pdu_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_pdu_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
