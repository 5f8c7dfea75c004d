"""GPU: FskTxMulti of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_tx.hip):
tests/cpp/test_fsk_multi_host.cpp pushes the rows and counts written here and writes every stream's audio and outputs back; they
must be rr.FskTxMulti's bit for bit (the same pushes give the same bits), with the counts of tests/fsk_model.py."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import fsk_model as fk
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("fskmcpp") / "test_fsk_multi_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_fsk_multi_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", e], check=True)
    return e


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
def test_cpp_mirror_fsk_tx_multi(exe, tmp_path, mode):
    N, i1, d1, i2, d2, n_cap = 3, 10, 1, 25, 24, 230
    lo, hi, gain, k1, k2 = 1200.0, 2200.0, 0.5, 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
    counts = [[n_cap, 0, 1], [7, n_cap + 50, 0], [205, 1, 204]]
    rows = [np.stack([fk.patterns(n_cap, 61 + 10 * p + c)["random"] for c in range(N)]) for p in range(len(counts))]
    vec, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<8Q3f2d", mode, N, i1, d1, i2, d2, n_cap, len(counts), lo, hi, gain, k1, k2))
        for k, r in zip(counts, rows):
            f.write(np.array(k, "<u8").tobytes() + r.tobytes())
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    afsk = mode == rr.FSK_TX_AFSK
    h = rr.FskTxMulti(N, mode, i1, d1, lo, hi, k1, gain, i2, d2, k2)
    r1, r2 = fk.reduced(i1, d1), fk.reduced(i2, d2)
    raw, at, taken = open(out, "rb").read(), 0, [[] for _ in range(N)]
    for k, r in zip(counts, rows):
        want = h.push(r, k, audio=True) if afsk else (h.push(r, k), None)
        for c in range(N):
            na, no = struct.unpack_from("<2Q", raw, at)
            at += 16
            taken[c].append(min(k[c], n_cap))
            assert (na, no) == fk.counts(taken[c], r1, r2)[-1]
            if afsk:
                a = np.frombuffer(raw, np.float32, na, at); at += 4 * na
                assert np.array_equal(a.view(np.uint32), want[1][c].view(np.uint32))
            o = np.frombuffer(raw, np.complex64, no, at); at += 8 * no
            assert np.array_equal(o.view(np.uint32), want[0][c].view(np.uint32))
    assert at == len(raw)
