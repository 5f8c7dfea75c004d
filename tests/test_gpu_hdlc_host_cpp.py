"""GPU: the deframer of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_hdlc.hip):
tests/cpp/test_hdlc_host.cpp pushes the bits written here, in the windows named here, and writes every frame back with its
packet_pos tag; frames, positions, repaired flags and counters must be the sequential model's, bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hdlc_model as hm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_deframer(tmp_path):
    rng = np.random.default_rng(71)
    bits = hm.draw_stream(rng, 30000)
    cfg = (1, 10, False, True)
    win = []
    while sum(win) < len(bits):
        win.append(min(int(rng.integers(1, 3000)), len(bits) - sum(win)))
    win.insert(3, 0)                                        # an empty push in between
    vec, out = tmp_path / "bits.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<QQQQQQ", cfg[0], cfg[1], int(cfg[2]), int(cfg[3]), len(bits), len(win)))
        f.write(bits.tobytes())
        f.write(np.array(win, "<u8").tobytes())
    exe = str(tmp_path / "test_hdlc_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_hdlc_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw = open(out, "rb").read()
    got, at = [], 0
    while True:
        pos, n, fixed = struct.unpack_from("<QQQ", raw, at)
        if pos == 2 ** 64 - 1:
            stats = (n, fixed, struct.unpack_from("<Q", raw, at + 24)[0])
            assert at + 32 == len(raw)
            break
        got.append((pos, raw[at + 24:at + 24 + n], bool(fixed)))
        at += 24 + n
    m = hm.HdlcModel(*cfg)
    want = m.run(bits)
    assert got == want and len(want) > 50
    assert stats == m.stats() and stats[2] > 10
