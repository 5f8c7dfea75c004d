"""GPU: AfskDemod of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_afsk.hip):
tests/cpp/test_afsk_host.cpp pushes the rows written here, in the windows named here, and writes every output back; the outputs
must be rr.AfskDemod's bit for bit and within the bound of the float64 definition."""
import os
import struct
import subprocess

import numpy as np
import pytest

import afsk_model as am
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_afsk_demod(tmp_path):
    ns, H, L, n = 3, 65, 289, 2 * 2048 + 3
    gain, off = 1.0, float(am.OFFSET)
    x = np.stack([am.two_tone(n, 30 + c) for c in range(ns)])
    taps = am.lp_taps(L)
    win = [1, 2047, 0, 100, n - 2148]
    vec, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<5Q2f", ns, H, L, n, len(win), gain, off))
        f.write(taps.tobytes() + x.tobytes() + np.array(win, "<u8").tobytes())
    exe = str(tmp_path / "test_afsk_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_afsk_host.cpp")
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
    want = rr.AfskDemod(ns, H, taps, gain, off).push(x)
    assert got.shape == want.shape == (ns, n - 1) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    hil = am.hilbert(H)
    for c in range(ns):
        assert am.used(got[c], am.chain_f64(x[c], hil, gain, taps, off), gain, taps) <= 1.0
