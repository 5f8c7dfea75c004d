"""GPU: Il2pReceiver of the C++ host mirror (rustradio_amd/host/rustradio.hpp -> C ABI -> kernels_il2p.hip):
tests/cpp/test_il2p_host.cpp runs the ragged pushes written here; records, counters and positions must be tests/il2p_model.py's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import il2p_cases as ic
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_on_a_fuzz_case(tmp_path):
    seed = next(s for s in ic.FUZZ_SEEDS if len(ic.fuzz_case(s)[0]) == 3)
    streams, pushes, allowed, invert = ic.fuzz_case(seed)
    want, stats, consumed = ic.expected(streams, pushes, allowed)
    assert sum(len(w) for w in want) >= 3
    vec, out = tmp_path / "pushes.bin", tmp_path / "out.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<4Q", len(streams), int(invert), allowed, len(pushes)))
        for a, (n_cap, counts) in zip(ic.host_rows(streams, pushes, invert), pushes):
            for c, k in enumerate(counts):
                f.write(struct.pack("<Q", k))
                f.write(a[c, :k].tobytes())
    exe = os.path.join(ROOT, "tests", "cpp", "test_il2p_host.bin")
    src = os.path.join(ROOT, "tests", "cpp", "test_il2p_host.cpp")
    lib = os.path.join(ROOT, "rustradio_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", src, "-L", lib, "-lrustradio_amd", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    res = subprocess.run([exe, str(vec), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().endswith("OK")
    raw = open(out, "rb").read()
    at = 0
    for k, w in enumerate(want):
        n = struct.unpack_from("<Q", raw, at)[0]
        rec = np.frombuffer(raw, rr.IL2P_HEADER, n, at + 8)
        assert ic.device_records(rec) == w, k
        at += 8 + 64 * n
    tail = struct.unpack_from("<%dQ" % (3 * len(streams) + 2), raw, at)
    assert [tuple(tail[3 * c:3 * c + 2]) for c in range(len(streams))] == stats
    assert [tail[3 * c + 2] for c in range(len(streams))] == consumed
    assert tuple(tail[-2:]) == rr.Il2pReceiver(1).dims()
