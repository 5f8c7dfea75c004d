"""No GPU: what rr.FskTxMulti (rr_fsk_tx_multi_*) says and computes without a device: the new symbols, every refusal
sentence of create and push, its host twin FskMultiHost and fsk_multi_bound under the host sanitizers (tests/cpp/emu_fsk_multi.cpp),
and the loop-back condition of the three-station GPU test on the models alone."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import fsk_model as fk
import fsk_multi_dev as fmd
import rustradio_amd as rr

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
NEW_SYMBOLS = ("rr_fsk_tx_multi_create", "rr_fsk_tx_multi_bound", "rr_fsk_tx_multi_push_dev", "rr_fsk_tx_multi_push",
               "rr_fsk_tx_multi_counts", "rr_fsk_tx_multi_counts_dev", "rr_fsk_tx_multi_positions", "rr_fsk_tx_multi_dims",
               "rr_hdlc_framer_produced_dev")
K1, K2 = 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
P = "fsk tx multi: "


def test_new_symbols_are_exported():
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s


CREATE_REFUSALS = [
    (dict(nstreams=0), "nstreams out of range"),
    (dict(nstreams=65536), "nstreams out of range"),
    (dict(nstreams=0, mode=2), "fsk tx: unknown mode"),                     # fsk_check's refusals come first
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


@pytest.mark.parametrize("kw,msg", CREATE_REFUSALS, ids=[f"{list(k)[-1]}-{i}" for i, (k, _) in enumerate(CREATE_REFUSALS)])
def test_create_refusals_come_before_any_device(kw, msg):
    """each with its sentence; without a device a VALID create says "no usable HIP device" (below), so these were said before one
    was looked for"""
    args = dict(nstreams=3, mode=rr.FSK_TX_AFSK, interp1=10, deci1=1, lo=1200.0, hi=2200.0, k1=K1, gain=0.5, interp2=4, deci2=1, k2=K2)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        rr.FskTxMulti(**args)


def test_no_cpu_fallback():
    """without a device the block refuses to exist; with one it is the native block"""
    import torch
    makes = (lambda: rr.FskTxMulti(3, rr.FSK_TX_AFSK, 10, 1, 1200.0, 2200.0, K1, 0.5, 4, 1, K2),
             lambda: rr.FskTxMulti(65535, rr.FSK_TX_DIRECT, 5, 1, -3000.0, 3000.0, K1, 0.5, 8, 1, float("nan")))
    for make in makes:
        if torch.cuda.is_available():
            assert make().name.startswith("Resampler>Map>Vco")
        else:
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fskm") / "emu_fsk_multi")
    fk.build_cpp("emu_fsk_multi.cpp", exe, SAN)
    return exe


def test_host_twin_equals_the_one_stream_twin_and_the_bound_is_the_maximum(emu):
    """under ASan and UBSan: FskMultiHost per stream against FskHost bit for bit (both modes, the five shapes, ragged counts, counts
    above n_cap, zeros, a row that ends with its count), and fsk_multi_bound against fsk_first over every pair of residues"""
    r = subprocess.run([emu], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fsk multi ok" in r.stdout, r.stdout + r.stderr


# label -> the sentence fsk_multi_check / fsk_multi_check_push / fsk_multi_check_counts returns (tests/cpp/emu_fsk_multi.cpp has
# the arguments); the GPU tests show that the handle says the same with nothing launched
SENTENCES = {
    "create ok": "ok", "create nstreams 0": "nstreams out of range", "create nstreams 65535": "ok",
    "create nstreams 65536": "nstreams out of range", "create mode": "fsk tx: unknown mode",
    "create interp1": "interpolation and decimation must be nonzero", "create ratio": "fsk tx: reduced ratio part above 2^31",
    "create lo": "fsk tx: lo and hi must be finite", "create hi": "fsk tx: lo and hi must be finite",
    "create gain": "fsk tx: gain must be finite", "create k1": "fsk tx: k1 and k2 must be finite",
    "create k2": "fsk tx: k1 and k2 must be finite", "create k2 direct": "ok",
    "push ok": "ok", "push ok no audio": "ok", "push ok empty": "ok",
    "push direct audio": P + "DIRECT mode has no audio output",
    "push bits_stride": P + "bits_stride below n_cap",
    "push out_stride": P + "out_stride below the outputs a stream can make",
    "push audio_stride": P + "audio_stride below the audio samples a stream can make",
    "push audio_stride unused": "ok",
    "push n_cap": P + "more than 2^30 bits of a stream in one push",
    "push audio total": P + "more than 2^30 audio samples of all streams in one push",
    "push out total": P + "more than 2^30 outputs of all streams in one push",
    "push out total fits": "ok",
    "push null bits": P + "null bit buffer", "push null out": P + "null output buffer",
    "push position": P + "output position beyond 2^62", "push position fits": "ok",
    "counts ok": "ok", "counts audio": P + "the device's counts exceed the bound of the push",
    "counts out": P + "the device's counts exceed the bound of the push",
}


def test_every_refusal_has_its_sentence(emu):
    r = subprocess.run([emu, "refusals"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split("|", 1) for line in r.stdout.splitlines())
    assert got == SENTENCES
    said = {v for v in SENTENCES.values() if v.startswith(P)}
    assert len(said) == 11                                 # each refusal of a push its own sentence, and the read-back's


def test_the_loop_back_condition_holds_on_the_models_for_all_three_stations():
    """the three packet sets behind rr_hdlc_framer(FCS | NRZI), each through the sequential chain's audio, zero-padded as the
    three-station GPU test pads it (a zeroed buffer behind a stream's own count), the float64 tone demodulator and the models of
    SymbolSync and HdlcReceiver: every set comes back whole, once, in order, stats (n, 0, 0), under padding of 0, 1, 777, 5000,
    16820, up to the longest stream's audio and up to the audio_cap of the framers' largest bound"""
    t = fk.LOOP_TX
    sets, bits = fmd.station_packets(), fmd.station_bits()
    assert all(len(p) <= 58 for ps in sets for p in ps)
    audio = [fk.seq_chain(fk.AFSK, b, [len(b)], t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])[0]
             for b in bits]
    assert [len(a) for a in audio] == [10 * len(b) for b in bits]
    longest = max(len(a) for a in audio)
    cap = 10 * max(fmd.framer_bound(ps) for ps in sets)
    assert cap >= longest and all(len(b) <= fmd.framer_bound(ps) for b, ps in zip(bits, sets))
    for a, ps in zip(audio, sets):
        for pad in sorted({0, 1, 777, 5000, 16820, longest - len(a), cap - len(a)}):
            got, stats = fk.loop_receive_model(fk.demod_f64(np.concatenate([a, np.zeros(pad, np.float32)])))
            assert got == ps, (len(ps), pad)
            assert stats == (len(ps), 0, 0), (len(ps), pad)
