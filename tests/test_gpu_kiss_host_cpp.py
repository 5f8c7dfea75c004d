"""GPU: KissDecode and KissEncode of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_kiss.hip):
tests/cpp/test_kiss_host.cpp decodes the pushes written here and re-encodes what it delivered; packets, tags, counters and the
re-encoded stream must be tests/kiss_model.py's byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kiss_model as km

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_decode_then_encode(tmp_path):
    rng = np.random.default_rng(71)
    max_len = 600
    parts = [km.draw_stream(rng, 700, special=0.4)]
    for i in range(30):
        parts.append(km.encode_one(km.draw_stream(rng, int(rng.integers(0, 500)), special=0.3), int(rng.integers(0, 16))))
    parts.append(bytes([km.FEND, 0x00]) + bytes(0x41 for _ in range(max_len)) + bytes([km.FEND]))       # one byte too long
    pushes = km.split(rng, b"".join(parts), 4) + [b""]
    m = km.ClosedDecoder(max_len)
    want = [(i, *p) for i, ps in enumerate(m.push(p) for p in pushes) for p in ps]
    assert len(want) >= 25 and m.stats()[4] >= 1 and m.stats()[2] >= 1
    vec, out = tmp_path / "pushes.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<QQ", max_len, len(pushes)))
        for p in pushes:
            f.write(struct.pack("<Q", len(p))); f.write(p)
    exe = os.path.join(ROOT, "tests", "cpp", "test_kiss_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_kiss_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw = open(out, "rb").read()
    at = 8
    got = []
    for _ in range(struct.unpack_from("<Q", raw, 0)[0]):
        push, pos, port, inb, n = struct.unpack_from("<5Q", raw, at)
        got.append((push, pos, port, inb, raw[at + 40:at + 40 + n]))
        at += 40 + n
    assert got == want
    n = struct.unpack_from("<Q", raw, at)[0]
    assert raw[at + 8:at + 8 + n] == km.encode([w[4] for w in want], [w[2] for w in want])
    assert struct.unpack_from("<5Q", raw, at + 8 + n) == m.stats()
