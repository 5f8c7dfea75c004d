"""GPU: AmDemod and AirspyDecode of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_am.hip):
tests/cpp/test_am_mirror.cpp pushes the rows written here, in the windows named here, and writes every output back; the outputs
must be rr.AmDemod's bit for bit, the host twin's bit for bit, and within the bound of the float64 definition."""
import os
import struct
import subprocess

import numpy as np
import pytest

import am_model as am
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_am_demod(tmp_path):
    ns, L, I, D, scale = 3, 289, 3, 7, 0.5
    T = rr.AmDemod(1, am.taps_for(L), I, D, scale).dims()[0]
    n = am.samples_for_outputs(2 * T + 3, I, D)
    x = np.stack([am.am_signal(n, 30 + c, amp=10.0 ** c) for c in range(ns)])
    taps = am.taps_for(L)
    at_tile = am.samples_for_outputs(T, I, D)
    win = [1, at_tile - 1, 0, 100, n - at_tile - 100]
    vec, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<6Qf", ns, L, I, D, n, len(win), scale))
        f.write(taps.tobytes() + x.tobytes() + np.array(win, "<u8").tobytes())
    exe = str(tmp_path / "test_am_mirror")
    src = os.path.join(ROOT, "tests", "cpp", "test_am_mirror.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw, at, parts = open(out, "rb").read(), 0, []
    for _ in win:
        k = struct.unpack_from("<Q", raw, at)[0]
        at += 8
        parts.append(np.frombuffer(raw, np.float32, ns * k, at).reshape(ns, k))
        at += 4 * ns * k
    assert at == len(raw)
    got = np.concatenate(parts, axis=1)
    want = rr.AmDemod(ns, taps, I, D, scale).push(x)
    assert got.shape == want.shape == (ns, am.count(n, I, D)) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), am.twin(x, taps, I, D, scale).view(np.uint32))
    for c in range(ns):
        assert am.used(got[c], am.chain_f64(x[c], taps, I, D, scale), L, scale) <= 1.0
