"""No GPU: the 8- and 16-point butterflies of rustradio_amd/csrc/fft_core.hpp (host forms, the algorithm the kernels run) as
a stand-alone program under -fsanitize=address,undefined (tests/cpp/test_fft_const_fold.cpp): forward and inverse, unit
impulses in every position (re and im) and 64 seeded random vectors against a direct DFT in double, within TOL = 1e-5 of the
output's max, and no worse than the unfolded butterflies (every constant rotation a product of its own) by more than one
f32 rounding.  Worst error / max, folded against unfolded, as the program prints them:
    dft8  forward 9.014e-08 / 1.007e-07    dft8  inverse 8.817e-08 / 1.098e-07
    dft16 forward 1.162e-07 / 1.187e-07    dft16 inverse 8.866e-08 / 1.062e-07"""
import subprocess

import fsk_model as fk

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_folded_butterflies_against_a_direct_dft(tmp_path):
    exe = str(tmp_path / "test_fft_const_fold")
    fk.build_cpp("test_fft_const_fold.cpp", exe, SAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "fft const fold ok" in r.stdout, r.stdout + r.stderr
