"""No GPU: the float64 definition of rr.AfskDemod (tests/afsk_model.py) against the oracle's Hilbert -> QuadratureDemod ->
FftFilterFloat, rustradio_amd/csrc/afsk_core.hpp tile by tile and thread by thread under the host sanitizers (tests/cpp/emu_afsk.cpp),
the conditions the end-to-end GPU test relies on, asserted on the models alone, and what the new entry points say without a device."""
import ctypes

import numpy as np
import pytest

import afsk_model as am
import harness
import rustradio_amd as rr
import symsync_model as sm
from oracle import pyoracle as orc

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("rr_add_const_f32_create", "rr_add_const_c32_create", "rr_afsk_demod_create", "rr_afsk_demod_push_dev",
               "rr_afsk_demod_push", "rr_afsk_demod_dims")
TILE = 2048                                   # AFSK_TILE (rr_afsk_demod_dims says it on a device)


def test_definition_equals_the_oracle_chain():
    """row 3 of the signal: float64 definition == run_chain([Hilbert, QuadratureDemod, FftFilterFloat]) + offset on the oracle's
    (shorter: FftFilterFloat withholds its last partial block) output, within the bound; the definition's count is T - 1"""
    x = am.samples()[0][3]
    taps = am.taps12k()
    assert len(taps) == 289
    ref = am.reference(3)
    assert len(ref["out"]) == len(x) - 1
    yo = harness.run_chain([orc.Hilbert(am.HIL), orc.QuadratureDemod(1.0), orc.FftFilterFloat(taps)], x)
    yo = yo.astype(np.float32) + np.float32(am.OFFSET)
    assert 0 < len(yo) <= len(x) - 1 and len(yo) > len(x) - 1 - 4096
    err = np.abs(yo.astype(np.float64) - ref["out"][:len(yo)])
    u = float(np.max(err / am.bound(ref, am.GAIN, taps)[:len(yo)]))
    print(f"definition vs oracle: {len(yo)} of {len(x) - 1} outputs, max abs err {err.max():.3e}, used {u:.4f}")
    assert u <= 1.0


def _splits(rng, n, k):
    """k random cut points of n samples, with pushes of 0 and 1 samples put in"""
    at = np.sort(rng.integers(0, n + 1, k))
    lens = np.diff(np.concatenate([[0], at, [n]])).tolist()
    i = int(rng.integers(0, len(lens)))
    if lens[i] > 2:                            # a 1-sample push and an empty one in front of a long one
        lens[i:i + 1] = [1, 0, lens[i] - 1]
    return [int(v) for v in lens]


EMU_SHAPES = [(3, 1, 1, 2 * TILE + 3), (65, 2, 2, 2 * TILE + 3), (65, 289, 3, 2 * TILE + 3), (65, 1205, 1, 2 * TILE + 3),
              (65, TILE + 1, 1, 2 * TILE + 3), (5, 9, 2, 70)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("afsk")
    exe = str(d / "emu_afsk")
    am.build_emu(exe, SAN)
    return exe, str(d)


@pytest.mark.parametrize("H,L,ns,n", EMU_SHAPES, ids=[f"H{h}-L{l}-N{s}" for h, l, s, _ in EMU_SHAPES])
def test_afsk_core_on_the_cpu(emu, H, L, ns, n):
    """the kernel's indexing on the host, under ASan and UBSan: one push, the first pushes of 1 / 2 / 0 samples, and seeded random
    splits with 0- and 1-sample pushes — every split the same bits as one push, stream c the same bits as a 1-stream handle, and
    all of it within the bound of float64"""
    exe, tmp = emu
    rng = np.random.default_rng(H * 10007 + L)
    x = np.stack([am.two_tone(n, c) for c in range(ns)])
    hil, taps, gain, off = am.hilbert(H), am.lp_taps(L), 1.0, -0.25
    splits = [[n], [1, 2, 0, n - 3], [TILE - 1 if n > TILE else n // 2] + [n - (TILE - 1 if n > TILE else n // 2)]]
    splits += [_splits(rng, n, k) for k in (2, 5)]
    if ns > 1:
        splits.append(None)                   # row 0 alone
    cases = [(x if s is not None else x[:1], hil, gain, taps, off, s if s is not None else [n]) for s in splits]
    res = am.run_emu(exe, tmp, cases, f"H{H}L{L}")
    whole = res[0][0]
    assert whole.shape == (ns, n - 1)
    for s, pushes in zip(splits, res):
        got = np.concatenate(pushes, axis=1)
        want = whole if s is not None else whole[:1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), s
    for c in range(ns):
        u = am.used(whole[c], am.chain_f64(x[c], hil, gain, taps, off), gain, taps)
        print(f"H {H} L {L} stream {c}: used {u:.4f}")
        assert u <= 1.0


@pytest.fixture(scope="module")
def signal_chain():
    """the float64 chain over the unpadded rows of the 16-stream signal, then the models in one push"""
    x, lens = am.samples()
    rows = [am.reference(c)["out"][:lens[c] - 1].astype(np.float32) for c in range(am.NSTREAMS)]
    return rows


def test_the_signal_decodes_on_the_models_alone(signal_chain):
    """all three payloads of all 16 streams with stats (3, 0, 0), in one push and in the three pushes [n//3 + 7, 64, rest]; the
    smallest |symbol| from symbol 100 to the last frame's end is at least 100 x the largest bound there (so equal frames on the
    GPU are no accident of the tolerance); |a| stays away from 0 behind the start-up"""
    x, lens = am.samples()
    taps = am.taps12k()
    smallest, min_a, worst_ratio = np.inf, np.inf, np.inf
    for c, row in enumerate(signal_chain):
        one = am.chain_model([row], [len(row)])
        cut = am.chain_model([row], am.cuts(len(row)))
        for run in (one, cut):
            frames = [f for push in run for f in push["frames"][0]]
            assert [f[1] for f in frames] == am.payloads(c), c
            assert run[-1]["stats"][0] == (3, 0, 0), c
        syms, _, idx = sm.SymbolSync(*am.SYNC_PRM).run(row)
        end = one[0]["frames"][0][-1][0]                          # the symbol that ended the last frame
        assert 100 < end <= len(syms)
        span = slice(100, end)
        ref = am.reference(c)
        b = am.bound(ref, am.GAIN, taps)[idx[span]]
        s = float(np.min(np.abs(syms[span])))
        smallest = min(smallest, s)
        worst_ratio = min(worst_ratio, s / float(np.max(b)))
        min_a = min(min_a, float(np.min(np.abs(ref["a"][2 * am.HIL:lens[c]]))))
    print(f"smallest |symbol| {smallest:.4f}, min |a| {min_a:.3f}, smallest |symbol| / largest bound {worst_ratio:.1f}")
    assert worst_ratio >= 100.0
    assert smallest > 0.2 and min_a > 0.3


def test_the_examples_clock_settings_lose_frames_at_ten_samples_per_symbol(signal_chain):
    """why the tests use (0.5, [0.1, 0.9]): with the example's (0.5, [0.5, 0.5]) fewer than half of the streams decode"""
    good = 0
    for c, row in enumerate(signal_chain):
        syms = sm.SymbolSync(10.0, 0.5, [0.5, 0.5]).run(row)[0]
        rx = am.hx.ModelReceiver(1, am.MAX_SIZE, nrzi=True)
        good += [f[1] for f in rx.push(syms)] == am.payloads(c)
    print(f"{good} of 16 decode with (0.5, [0.5, 0.5])")
    assert good < 8


def test_new_symbols_are_exported():
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s


REFUSALS = [
    (dict(nstreams=0), "nstreams out of range"),
    (dict(nstreams=4097), "nstreams out of range"),
    (dict(hilbert_ntaps=64), "hilbert filter len must be odd and greater than 1"),
    (dict(hilbert_ntaps=1), "hilbert filter len must be odd and greater than 1"),
    (dict(hilbert_ntaps=1025), "hilbert filter len above 1023"),
    (dict(window=7), "unknown window"),
    (dict(taps=[]), "AfskDemod needs 1 to 4096 finite taps"),
    (dict(taps=np.ones(4097, np.float32)), "AfskDemod needs 1 to 4096 finite taps"),
    (dict(taps=[0.5, np.nan]), "AfskDemod needs 1 to 4096 finite taps"),
    (dict(taps=[np.inf]), "AfskDemod needs 1 to 4096 finite taps"),
    (dict(gain=np.nan), "gain and offset must be finite"),
    (dict(offset=np.inf), "gain and offset must be finite"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[f"{list(k)[0]}-{i}" for i, (k, _) in enumerate(REFUSALS)])
def test_create_refusals_come_before_any_device(kw, msg):
    """each with its sentence; without a device a VALID create says "no usable HIP device", so these were said before one was
    looked for"""
    args = dict(nstreams=2, hilbert_ntaps=65, taps=[0.25, 0.5, 0.25], gain=1.0, offset=0.0, window=rr.WIN_HAMMING)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        rr.AfskDemod(**args)


def test_no_cpu_fallback():
    """without a device the new blocks refuse to exist; with one they are the native blocks"""
    import torch
    makes = (lambda: rr.AfskDemod(2, 65, [1.0]), lambda: rr.AddConst(1.0), lambda: rr.AddConst(1 + 2j, np.complex64))
    for make in makes:
        if torch.cuda.is_available():
            assert make().name in ("AddConst", "Hilbert>QuadratureDemod>FftFilterFloat>AddConst")
        else:
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
