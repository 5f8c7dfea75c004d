"""No GPU: the float64 definition of rr.AmDemod (tests/am_model.py) against the oracle's FftFilterFloat -> RationalResampler ->
MultiplyConst over np.hypot magnitudes, the magnitude's bits, rustradio_amd/csrc/am_core.hpp tile by tile and thread by thread
under the host sanitizers (tests/cpp/emu_am.cpp), every refusal sentence without a device (tests/cpp/test_am_host.cpp), the
conditions the end-to-end GPU test relies on, asserted on the model alone, and what the new entry points say without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import am_model as am
import harness
import rustradio_amd as rr
from oracle import pyoracle as orc

NEW_SYMBOLS = ("rr_am_demod_create", "rr_am_demod_push_dev", "rr_am_demod_push", "rr_am_demod_dims", "rr_airspy_decode_create")


@pytest.mark.parametrize("I,D", [(3, 7), (1, 1)], ids=["3to7", "1to1"])
def test_definition_equals_the_oracle_chain(I, D):
    """float64 definition == run_chain([FftFilterFloat, RationalResampler, MultiplyConst]) over np.hypot magnitudes at 289 taps,
    on the oracle's (shorter: FftFilterFloat withholds its last partial block) output, within B[o] + 1e-5 max|y| (the allowance
    tests/afsk_model.py gives this same oracle filter)"""
    L, scale, n = 289, 0.75, 20000
    x = am.am_signal(n, 1)
    taps = am.lp_taps(L)
    m = np.hypot(x.real, x.imag)
    assert m.dtype == np.float32
    yo = harness.run_chain([orc.FftFilterFloat(taps), orc.RationalResampler(I, D, np.float32), orc.MultiplyConst(scale)], m)
    ref = am.chain_f64(x, taps, I, D, scale)
    assert len(ref["out"]) == am.count(n, I, D)
    assert 0 < len(yo) <= len(ref["out"]) and len(yo) > len(ref["out"]) - am.count(8192, I, D)
    short = {k: v[:len(yo)] for k, v in ref.items()}
    u = am.used(yo, short, L, scale, extra=1e-5 * float(np.max(np.abs(ref["out"]))))
    print(f"definition vs oracle {I}:{D}: {len(yo)} of {len(ref['out'])} outputs, used {u:.4f}")
    assert u <= 1.0


def test_magnitude_is_hypotf():
    """np.hypot in f32 (glibc's hypotf) == fl32(sqrt(f64(re)^2 + f64(im)^2)) bit for bit: 2^20 random pairs spanning 2^+-30 and
    every int16 AirSPY value against a spread of partners"""
    rng = np.random.default_rng(5)
    n = 1 << 20
    re = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)).astype(np.float32)
    im = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)).astype(np.float32)
    x = re + 1j * im
    assert np.array_equal(np.hypot(re, im).view(np.uint32), am.mag32(x.astype(np.complex64)).view(np.uint32))
    v = (np.arange(-32768, 32768).astype(np.float32) / np.float32(1000))
    for q in (-32768, -12345, -1, 0, 1, 777, 20011, 32767):
        w = np.full_like(v, np.float32(q) / np.float32(1000))
        for a, b in ((v, w), (w, v)):
            assert np.array_equal(np.hypot(a, b).view(np.uint32), am.mag32((a + 1j * b).astype(np.complex64)).view(np.uint32))
    rv = rng.integers(-32768, 32768, (2, n)).astype(np.float32) / np.float32(1000)
    assert np.array_equal(np.hypot(rv[0], rv[1]).view(np.uint32), am.mag32((rv[0] + 1j * rv[1]).astype(np.complex64)).view(np.uint32))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("am")
    exe = str(d / "emu_am")
    am.build_emu(exe, am.SAN)
    return exe, str(d)


# (L, I, D, nstreams, n); n as a function of T = dims()[0]
EMU_SHAPES = [
    (1, 1, 1, 1, lambda T: 2 * T + 3),
    (2, 1, 1, 2, lambda T: 2 * T + 3),
    (289, 3, 7, 3, lambda T: 7 * T + 5),
    (33, 5, 2, 2, lambda T: 300),
    (9, 1, 1000, 2, lambda T: 5000),
    (12045, 12, 625, 1, lambda T: am.samples_for_outputs(2 * T + 1, 12, 625)),
    (16384, 1, 1, 1, lambda T: T + 2),
]


@pytest.mark.parametrize("L,I,D,ns,nf", EMU_SHAPES, ids=[f"L{s[0]}-{s[1]}to{s[2]}-N{s[3]}" for s in EMU_SHAPES])
def test_am_core_on_the_cpu(emu, L, I, D, ns, nf):
    """the kernel's indexing on the host, under ASan and UBSan: one push, first pushes of 1 / 2 / 0 samples, a cut on a tile's
    last output, and seeded random splits with 0- and 1-sample pushes — every split the same bits as one push, stream c the same
    bits as a 1-stream handle, and all of it within the bound of float64"""
    exe, tmp = emu
    T, C = am.emu_dims(exe, L, I, D)
    assert C == L - 1 and 32 <= T <= 192
    n = nf(T)
    rng = np.random.default_rng(L * 10007 + D)
    x = np.stack([am.am_signal(n, c, amp=10.0 ** c) for c in range(ns)])
    taps, scale = am.taps_for(L), 0.5
    at_tile = min(am.samples_for_outputs(T, I, D), n - 1)
    splits = [[n], [1, 2, 0, n - 3], [at_tile, n - at_tile]]
    splits += [am.split_lens(rng, n, k) for k in (2, 5)]
    if ns > 1:
        splits.append(None)                   # row 0 alone
    cases = [(x if s is not None else x[:1], taps, I, D, scale, s if s is not None else [n]) for s in splits]
    res = am.run_emu(exe, tmp, cases, f"L{L}D{D}")
    whole = res[0][0]
    assert whole.shape == (ns, am.count(n, I, D))
    for s, pushes in zip(splits, res):
        got = np.concatenate(pushes, axis=1)
        want = whole if s is not None else whole[:1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), s
    for c in range(ns):
        u = am.used(whole[c], am.chain_f64(x[c], taps, I, D, scale), L, scale)
        print(f"L {L} {I}:{D} stream {c}: used {u:.4f}")
        assert u <= 1.0


def test_every_refusal_sentence_without_a_device(tmp_path):
    """tests/cpp/test_am_host.cpp: am_host.hpp's create and push refusals, compiled alone (no HIP, no library)"""
    exe = str(tmp_path / "test_am_host")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *am.SAN, "-I", os.path.join(am.ROOT, "rustradio_amd", "csrc"),
                    os.path.join(am.ROOT, "tests", "cpp", "test_am_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "am host ok" in r.stdout, r.stdout + r.stderr


def test_the_three_stations_separate_on_the_model_alone():
    """the end-to-end signal through the float64 model: each channel's audio, mean removed, correlates above 0.99 with its own
    station's tone and below 0.2 with the other two"""
    s = am.e2e_scores(am.e2e_model())
    print(np.round(s, 4))
    for c in range(3):
        for t in range(3):
            assert (s[c, t] > 0.99) if c == t else (s[c, t] < 0.2), (c, t, s[c, t])


def test_new_symbols_are_exported_and_declared():
    L = ctypes.CDLL(rr.LIB_PATH)
    header = open(os.path.join(am.ROOT, "include", "rustradio_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
        assert re.search(r"\b" + s + r"\(", header), s


REFUSALS = [
    (dict(nstreams=0), "nstreams out of range"),
    (dict(nstreams=4097), "nstreams out of range"),
    (dict(taps=[]), "AmDemod needs 1 to 16384 finite taps"),
    (dict(taps=np.ones(16385, np.float32)), "AmDemod needs 1 to 16384 finite taps"),
    (dict(taps=[0.5, np.nan]), "AmDemod needs 1 to 16384 finite taps"),
    (dict(taps=[np.inf]), "AmDemod needs 1 to 16384 finite taps"),
    (dict(deci=0), "RationalResampler created using deci 0"),
    (dict(interp=0), "RationalResampler created using interp 0"),
    (dict(interp=2 ** 31 + 1, deci=1), "am demod: reduced ratio part above 2\\^31"),
    (dict(interp=1, deci=2 ** 32 + 1), "am demod: reduced ratio part above 2\\^31"),
    (dict(scale=np.nan), "scale must be finite"),
    (dict(scale=np.inf), "scale must be finite"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[f"{list(k)[0]}-{i}" for i, (k, _) in enumerate(REFUSALS)])
def test_create_refusals_come_before_any_device(kw, msg):
    """each with its sentence; without a device a VALID create says "no usable HIP device", so these were said before one was
    looked for"""
    args = dict(nstreams=2, taps=[0.25, 0.5, 0.25], interp=1, deci=1, scale=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        rr.AmDemod(**args)


def test_no_cpu_fallback():
    """without a device the new blocks refuse to exist; with one they are the native blocks"""
    import torch
    makes = (lambda: rr.AmDemod(2, [1.0]), lambda: rr.AirspyDecode())
    for make in makes:
        if torch.cuda.is_available():
            assert make().name in ("AirspyDecode", "Norm>FftFilterFloat>RationalResampler>MultiplyConst")
        else:
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
