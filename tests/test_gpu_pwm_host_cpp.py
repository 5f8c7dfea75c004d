"""GPU: PwmDecoder of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_pwm.hip):
tests/cpp/test_pwm_host.cpp pushes the Complex samples written here, in the windows named here, and writes every frame back; bits,
repeats, first_sample, order and the delivering push must be the sequential model's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pwm_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_pwm_decoder(tmp_path):
    rng = np.random.default_rng(11)
    short, long, fgap, rgap, nbits, min_repeats = 6, 20, 28, 230, 12, 2
    env = [np.zeros(700, np.float32)]
    for t in range(4):                                       # transmissions of 1 .. 4 repeats: the first stays below min_repeats
        bits = rng.integers(0, 2, nbits)
        for _ in range(t + 1):
            for b in bits:
                env += [np.ones(short if b else long, np.float32), np.zeros(long if b else short, np.float32)]
            env += [np.ones(short, np.float32), np.zeros(60, np.float32)]
        env.append(np.zeros(rgap if t < 3 else 100, np.float32))      # the last one is left to finish()
    env = np.concatenate(env)
    z = (env + rng.normal(0, 0.04, len(env)) + 1j * rng.normal(0, 0.04, len(env))).astype(np.complex64)
    win = []
    while sum(win) < len(z):
        win.append(min(int(rng.integers(1, 900)), len(z) - sum(win)))
    win.insert(2, 0)                                         # an empty push in between
    vec, out = tmp_path / "samples.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<9Q", short, long, fgap, rgap, nbits, min_repeats, 1, len(z), len(win)))
        f.write(z.tobytes())
        f.write(np.array(win, "<u8").tobytes())
    exe = str(tmp_path / "test_pwm_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_pwm_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw, got, at = open(out, "rb").read(), [], 0
    while at < len(raw):
        push, first, repeats, n = struct.unpack_from("<4Q", raw, at)
        got.append((push, tuple(raw[at + 32:at + 32 + n]), repeats, first))
        at += 32 + n
    m = pm.PwmModel(0.5, short, long, fgap, rgap, frame_bits=nbits, min_repeats=min_repeats, delimiter=True)
    zr, zi = z.real.astype(np.float32), z.imag.astype(np.float32)
    power, want, at = (zr * zr + zi * zi).astype(np.float32), [], 0
    for k, w in enumerate(win):
        want += [(k, *f) for f in m.push(power[at:at + w])]
        at += w
    want += [(len(win), *f) for f in m.flush()]
    assert got == want
    assert [f[2] for f in want] == [2, 3, 4] and want[-1][0] == len(win)
