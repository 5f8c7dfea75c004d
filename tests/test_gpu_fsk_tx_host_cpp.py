"""GPU: FskTx of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_tx.hip): tests/cpp/test_fsk_host.cpp
pushes the bits written here, in the pushes named here, and writes every audio sample and output back; they must be rr.FskTx's bit
for bit (the same pushes give the same bits) and within the bounds of tests/fsk_model.py."""
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
    e = str(tmp_path_factory.mktemp("fskcpp") / "test_fsk_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_fsk_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", e], check=True)
    return e


@pytest.mark.parametrize("mode", [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT], ids=["afsk", "direct"])
def test_cpp_mirror_fsk_tx(exe, tmp_path, mode):
    i1, d1, i2, d2, n = 10, 1, 25, 24, 450
    lo, hi, gain, k1, k2 = 1200.0, 2200.0, 0.5, 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
    bits = fk.patterns(n, 61)["random"]
    lens = [1, 204, 0, 205, n - 410]
    vec, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<7Q3f2d", mode, i1, d1, i2, d2, n, len(lens), lo, hi, gain, k1, k2))
        f.write(bits.tobytes() + np.array(lens, "<u8").tobytes())
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw, at, auds, outs = open(out, "rb").read(), 0, [], []
    for _ in lens:
        na, no = struct.unpack_from("<2Q", raw, at)
        at += 16
        if mode == rr.FSK_TX_AFSK:
            auds.append(np.frombuffer(raw, np.float32, na, at)); at += 4 * na
        outs.append(np.frombuffer(raw, np.complex64, no, at)); at += 8 * no
    assert at == len(raw)
    got = np.concatenate(outs)
    h = rr.FskTx(mode, i1, d1, lo, hi, k1, gain, i2, d2, k2)
    r1, r2 = fk.reduced(i1, d1), fk.reduced(i2, d2)
    want_o, want_a, pos = [], [], 0
    for k in lens:
        r = h.push(bits[pos:pos + k], audio=mode == rr.FSK_TX_AFSK)
        want_o.append(r[0] if mode == rr.FSK_TX_AFSK else r)
        if mode == rr.FSK_TX_AFSK:
            want_a.append(r[1])
        pos += k
    assert np.array_equal(got.view(np.uint32), np.concatenate(want_o).view(np.uint32))
    if mode == rr.FSK_TX_AFSK:
        audio = np.concatenate(auds)
        assert np.array_equal(audio.view(np.uint32), np.concatenate(want_a).view(np.uint32))
        ua, _ = fk.used_audio(audio, bits, r1, lo, hi, k1, gain)
        uo, _ = fk.used_out(got, audio, r2, k2)
    else:
        ua, _ = fk.used_direct(got, fk.made(n, *r1), bits, r1, r2, lo, hi, k1, gain)
        uo = 0.0
    assert ua <= 1.0 and uo <= 1.0
