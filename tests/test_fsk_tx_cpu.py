"""No GPU: the reference's transmit chains restated one sample after the other (tests/fsk_model.py) against the closed forms and the
three bounds of rr.FskTx, the run-length form of rustradio_amd/csrc/fsk_core.hpp under the host sanitizers (tests/cpp/emu_fsk.cpp)
against the same bounds, the index arithmetic against brute force and Python integers (tests/cpp/test_fsk_hostlogic.cpp), the
condition of the loop-back GPU tests on the models alone, and what the new entry points say without a device."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import fsk_model as fk
import rustradio_amd as rr

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("rr_fsk_tx_create", "rr_fsk_tx_count", "rr_fsk_tx_push_dev", "rr_fsk_tx_push", "rr_fsk_tx_dims")
K1, K2 = 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
# (i1, d1, i2, d2): the issue's four, and 1:1 / 1:1
SHAPES = [(10, 1, 4, 1), (40, 1, 25, 24), (3, 7, 3, 7), (7, 3, 4099, 1), (1, 1, 1, 1)]
IDS = [f"{a}:{b}-{c}:{d}" for a, b, c, d in SHAPES]


def _nbits(i1, d1, i2, d2, audio=3000):
    """bits for about `audio` audio samples, fewer where the second ratio makes many outputs of each"""
    audio = min(audio, max(8, 200000 * d2 // i2))
    return max(4, audio * d1 // i1)


def _tx(mode, sh, lo=1200.0, hi=2200.0, k1=K1, gain=0.5, k2=K2):
    i1, d1, i2, d2 = sh
    return (mode, i1, d1, lo, hi, k1, gain, i2, d2, k2)


@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_sequential_chain_has_the_closed_forms_indices_and_counts(sh):
    """the counter loop against out[m] = in[floor(m D / I)] and ceil(N I / D), for the shapes and for random ratios and splits"""
    rng = np.random.default_rng(sum(sh))
    ratios = [(sh[0], sh[1]), (sh[2], sh[3])] + [(int(rng.integers(1, 60)), int(rng.integers(1, 60))) for _ in range(6)]
    for i, d in ratios:
        n = int(rng.integers(1, 300))
        x = list(range(n))
        sp = fk.splits(rng, n, 4)
        rs, got, at = fk.Resampler(i, d), [], 0
        ri, rd = fk.reduced(i, d)
        for k in sp:
            part = rs.push(x[at:at + k])
            assert len(part) == fk.made(at + k, ri, rd) - fk.made(at, ri, rd)          # every push: everything its inputs produce
            got += part
            at += k
        assert got == [fk.src(m, ri, rd) for m in range(fk.made(n, ri, rd))]
        for k in range(n):
            assert got[fk.first(k, ri, rd):fk.first(k + 1, ri, rd)] == [k] * fk.rep(k, ri, rd)


def _check(mode, tx, bits, audio, out, label):
    _, i1, d1, lo, hi, k1, gain, i2, d2, k2 = tx
    r1, r2 = fk.reduced(i1, d1), fk.reduced(i2, d2)
    if mode == fk.AFSK:
        ua, ta = fk.used_audio(audio, bits, r1, lo, hi, k1, gain)
        uo, to = fk.used_out(out, audio, r2, k2)
    else:
        ua, ta = fk.used_direct(out, fk.made(len(bits), *r1), bits, r1, r2, lo, hi, k1, gain)
        uo, to = 0.0, 0.0
    print(f"{label}: used {ua:.4f} (stage 1 / DIRECT), {uo:.4f} (AFSK out); the truths' own error {ta:.2e}, {to:.2e} of the bound")
    assert ta <= 0.01 and to <= 0.01
    assert ua <= 1.0 and uo <= 1.0
    return max(ua, uo)


@pytest.mark.parametrize("mode", [fk.AFSK, fk.DIRECT], ids=["afsk", "direct"])
@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_sequential_chain_meets_the_bounds(sh, mode):
    """the reference's f64 recurrences, whole and in random splits (the same samples: its state is carried exactly)"""
    n = _nbits(*sh, audio=1500)
    bits = fk.patterns(n, 5)["random"]
    tx = _tx(mode, sh)
    audio, out, cnt = fk.seq_chain(mode, bits, [n], *tx[1:])
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    assert cnt == fk.counts([n], r1, r2)
    sp = fk.splits(np.random.default_rng(n), n, 5)
    a2, o2, c2 = fk.seq_chain(mode, bits, sp, *tx[1:])
    assert c2 == fk.counts(sp, r1, r2)
    assert np.array_equal(o2.view(np.uint32), out.view(np.uint32)) and np.array_equal(a2.view(np.uint32), audio.view(np.uint32))
    _check(mode, tx, bits, audio if mode == fk.AFSK else None, out, "sequential")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("fsk")
    exe = str(d / "emu_fsk")
    fk.build_cpp("emu_fsk.cpp", exe, SAN)
    return exe, str(d)


@pytest.mark.parametrize("sh", SHAPES, ids=IDS)
def test_run_length_form_on_the_cpu(emu, sh):
    """fsk_core.hpp's arithmetic (counts -> phase 1, weights rep2 -> phase 2, j d inside a run) under ASan and UBSan, both modes,
    the four bit patterns, whole and split: the counts of the closed forms, every result within the bounds, and large steps"""
    exe, tmp = emu
    n = _nbits(*sh)
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    rng = np.random.default_rng(n + sh[2])
    cases, labels = [], []
    for name, bits in fk.patterns(n, 11).items():
        for mode in (fk.AFSK, fk.DIRECT):
            for sp in ([n], fk.splits(rng, n, 6), [1, 1, 0, 2, n - 4]):
                cases.append((*_tx(mode, sh)[:1], bits, sp, *_tx(mode, sh)[1:]))
                labels.append(f"{name} {'afsk' if mode else 'direct'} {len(sp)} pushes")
    big = fk.patterns(n, 12)["random"]
    cases.append((fk.AFSK, big, [n], sh[0], sh[1], -1.0, 1.0, 14.2, 0.5, sh[2], sh[3], K2))      # |k1 hi| > 4 pi
    cases.append((fk.AFSK, big, [n], sh[0], sh[1], 1200.0, 2200.0, K1, 0.5, sh[2], sh[3], 9.5 * math.pi))  # |k2 gain| > 4 pi
    cases.append((fk.DIRECT, big, [n], sh[0], sh[1], -1.0, 1.0, -14.2, 2.0, sh[2], sh[3], 0.0))
    labels += ["large k1", "large k2", "large k1 direct"]
    worst = 0.0
    for case, label, (audio, out, cnt) in zip(cases, labels, fk.run_emu(exe, tmp, cases, "s" + "_".join(map(str, sh)))):
        mode, bits, sp = case[0], case[1], case[2]
        assert cnt == fk.counts(sp, r1, r2), label
        tx = (mode, *case[3:])
        worst = max(worst, _check(mode, tx, bits, audio if mode == fk.AFSK else None, out, label))
    print(f"worst used fraction {worst:.4f}")


def test_run_length_form_equals_the_sequential_chain_where_nothing_rounds_differently(emu):
    """the two forms against each other: not bit-identical by contract, but both inside the bound, so at most two bounds apart"""
    exe, tmp = emu
    sh, n = (10, 1, 4, 1), 300
    bits = fk.patterns(n, 3)["random"]
    tx = _tx(fk.AFSK, sh)
    audio, out, _ = fk.seq_chain(fk.AFSK, bits, [n], *tx[1:])
    (a2, o2, _), = fk.run_emu(exe, tmp, [(fk.AFSK, bits, [n], *tx[1:])], "both")
    d1 = fk.d1_of(1200.0, 2200.0, K1)
    assert np.all(np.abs(a2.astype(np.float64) - audio) <= 2.0 * fk.audio_bound(np.arange(len(audio)), 0.5, d1))
    # (the outputs follow each form's OWN audio, so they are compared through their truths above, not with each other)
    assert len(o2) == len(out)


@pytest.fixture(scope="module")
def hostlogic(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fskhl") / "test_fsk_hostlogic")
    fk.build_cpp("test_fsk_hostlogic.cpp", exe, SAN)
    return exe


def test_index_arithmetic_against_brute_force(hostlogic):
    r = subprocess.run([hostlogic], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fsk hostlogic ok" in r.stdout, r.stdout + r.stderr


def test_carried_positions_against_python_integers(hostlogic):
    """fsk_seek / fsk_plan at stream positions up to 2^62, ratios up to coprime parts near 2^31"""
    rng = np.random.default_rng(62)
    big = [2147483647, 2147483648, 2147483629, 2147483587]
    cases = []
    for _ in range(40):
        pick = lambda: int(rng.choice(big)) if rng.random() < 0.4 else int(rng.integers(1, 5000))
        i1, d1, i2, d2 = pick(), pick(), pick(), pick()
        r1, r2 = fk.reduced(i1, d1), fk.reduced(i2, d2)
        grow = max(1, -(-r1[0] // r1[1])) * max(1, -(-r2[0] // r2[1]))
        pos = int(rng.integers(0, 1 << 62)) // grow // 2                           # the outputs stay below 2^62
        n = int(rng.integers(0, max(2, min(1 << 30, (1 << 29) // grow))))
        cases.append((i1, d1, i2, d2, pos, n))
    cases.append((1, 1, 1, 1, (1 << 62) - 5, 5))
    for i1, d1, i2, d2, pos, n in cases:
        r = subprocess.run([hostlogic, "seek", *map(str, (i1, d1, i2, d2, pos, n))], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        got = [int(v) for v in r.stdout.split()]
        r1, r2 = fk.reduced(i1, d1), fk.reduced(i2, d2)
        a0, a1 = fk.made(pos, *r1), fk.made(pos + n, *r1)
        o0, o1 = fk.made(a0, *r2), fk.made(a1, *r2)
        want = [a0, o0, a0 * r1[1] - pos * r1[0], o0 * r2[1] - a0 * r2[0], a1 - a0, o1 - o0, a1, o1,
                a1 * r1[1] - (pos + n) * r1[0], o1 * r2[1] - a1 * r2[0]]
        assert got == want, (i1, d1, i2, d2, pos, n)


def test_the_loop_back_condition_holds_on_the_models_alone():
    """the chosen packets behind rr_hdlc_framer(FCS | NRZI), through the sequential chain's AUDIO, the float64 tone demodulator and
    the models of SymbolSync and HdlcReceiver: every packet once, in order, CRC good, stats (npackets, 0, 0).  And through the
    chain's RF output: a float64 quadrature demodulator and every fourth sample give the audio back to within 1e-3."""
    bits = fk.loop_bits()
    t = fk.LOOP_TX
    audio, out, _ = fk.seq_chain(fk.AFSK, bits, [len(bits)], t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])
    assert len(audio) == 10 * len(bits) and len(out) == 4 * len(audio)
    got, stats = fk.loop_receive_model(fk.demod_f64(audio))
    assert got == fk.loop_packets()
    assert stats == (len(got), 0, 0)
    # out = (sin p2, cos p2) = j e^(-j p2): arg(conj(prev) * cur) = -(p2[o] - p2[o - 1]) = -k2 a
    z = out.astype(np.complex128)
    rf = -np.angle(z[1:] * np.conj(z[:-1])) / t["k2"]
    back = rf[3::4]                                                    # output 4 m + 4 - 1 ... the last step into each run
    assert np.max(np.abs(back[:len(audio) - 1] - audio[1:len(back) + 1])) < 1e-3
    got, stats = fk.loop_receive_model(fk.demod_f64(back))
    assert got == fk.loop_packets() and stats == (len(got), 0, 0)


def test_new_symbols_are_exported():
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s


CREATE_REFUSALS = [
    (dict(mode=2), "fsk tx: unknown mode"),
    (dict(mode=-1), "fsk tx: unknown mode"),
    (dict(interp1=0), "interpolation and decimation must be nonzero"),
    (dict(deci1=0), "interpolation and decimation must be nonzero"),
    (dict(interp2=0), "interpolation and decimation must be nonzero"),
    (dict(deci2=0), "interpolation and decimation must be nonzero"),
    (dict(interp1=(1 << 31) + 1), "fsk tx: reduced ratio part above 2\\^31"),
    (dict(deci2=(1 << 33) + 1), "fsk tx: reduced ratio part above 2\\^31"),
    (dict(lo=np.nan), "fsk tx: lo and hi must be finite"),
    (dict(hi=np.inf), "fsk tx: lo and hi must be finite"),
    (dict(gain=np.nan), "fsk tx: gain must be finite"),
    (dict(k1=np.inf), "fsk tx: k1 and k2 must be finite"),
    (dict(k2=np.nan), "fsk tx: k1 and k2 must be finite"),
]


@pytest.mark.parametrize("kw,msg", CREATE_REFUSALS, ids=[f"{list(k)[0]}-{i}" for i, (k, _) in enumerate(CREATE_REFUSALS)])
def test_create_refusals_come_before_any_device(kw, msg):
    """each with its sentence; without a device a VALID create says "no usable HIP device" (below), so these were said before one
    was looked for"""
    args = dict(mode=rr.FSK_TX_AFSK, interp1=10, deci1=1, lo=1200.0, hi=2200.0, k1=K1, gain=0.5, interp2=4, deci2=1, k2=K2)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        rr.FskTx(**args)


def test_no_cpu_fallback():
    """without a device the block refuses to exist; with one it is the native block"""
    import torch
    makes = (lambda: rr.FskTx(rr.FSK_TX_AFSK, 10, 1, 1200.0, 2200.0, K1, 0.5, 4, 1, K2),
             lambda: rr.FskTx(rr.FSK_TX_DIRECT, 5, 1, -3000.0, 3000.0, K1, 0.5, 8, 1, float("nan")))
    for make in makes:
        if torch.cuda.is_available():
            assert make().name.startswith("Resampler>Map>Vco")
        else:
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
