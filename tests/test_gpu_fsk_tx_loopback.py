"""GPU: packets through the library's own transmitter into its own receiver, on device pointers on one HIP stream, with
afsk_model's receive parameters (12 kS/s, 10 samples per symbol, SYNC_PRM, 289 taps):
  HdlcFramer(FCS | NRZI) -> FskTx(AFSK, 10:1, 1200, 2200, 2 pi / 12000, 0.5, 4:1, 2 pi 5000 / 48000)
  audio loop:  d_audio -> AfskDemod(1) -> SymbolSync -> HdlcReceiver(nrzi)
  RF loop:     out -> QuadratureDemod -> RationalResampler(1, 4) -> the same three blocks
Every packet comes back once, in order, CRC good, stats (npackets, 0, 0); tests/test_fsk_tx_cpu.py shows the same on the models."""
import numpy as np
import pytest
import torch

import afsk_model as am
import fsk_model as fk
import rustradio_amd as rr

pytestmark = pytest.mark.gpu


def stream0():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def transmitted():
    """-> (audio f32 tensor, out c64 tensor, n_bits) of the packets, both still on the device"""
    packets = fk.loop_packets()
    fr = rr.HdlcFramer(fk.LOOP_FLAGS)
    lens = np.array([len(p) for p in packets], np.uintp)
    starts = (np.cumsum(lens) - lens).astype(np.uintp)
    cap = fr.bound(lens)
    d_bytes = torch.from_numpy(np.frombuffer(b"".join(packets), np.uint8).copy()).cuda()
    d_bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream0()
    fr.push_dev(d_bytes.data_ptr(), int(lens.sum()), starts, lens, d_bits.data_ptr(), cap, s)
    _, n_bits = fr.records()                   # the one read of the host: the stuffing decides the count
    assert n_bits == len(fk.loop_bits())
    t = fk.LOOP_TX
    tx = rr.FskTx(rr.FSK_TX_AFSK, t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])
    na, no = tx.count(n_bits)
    assert (na, no) == (10 * n_bits, 40 * n_bits)
    audio = torch.zeros(na, dtype=torch.float32, device="cuda")
    out = torch.zeros(no, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    assert tx.push_dev(d_bits.data_ptr(), n_bits, out.data_ptr(), no, audio.data_ptr(), na, s) == (no, na)
    tx.sync()
    assert np.array_equal(d_bits[:n_bits].cpu().numpy(), fk.loop_bits())
    return audio, out, n_bits


def receive(d_audio, n):
    """AfskDemod(1) -> SymbolSync -> HdlcReceiver(nrzi) over n device samples -> ([payload], stats)"""
    af = rr.AfskDemod(1, am.HIL, am.taps12k(), am.GAIN, am.OFFSET)
    ss = rr.SymbolSync(*am.SYNC_PRM, nstreams=1)
    rx = rr.HdlcReceiver(1, 1, am.MAX_SIZE, nrzi=True)
    soft = torch.zeros(n, dtype=torch.float32, device="cuda")
    syms = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = stream0()
    p = af.push_dev(d_audio.data_ptr(), n, n, soft.data_ptr(), n, s)
    ss.push_dev(soft.data_ptr(), n, p, syms.data_ptr(), None, n, s)
    rx.push_dev(syms.data_ptr(), n, p, ss.counts_dev(), s)
    frames = [f[1] for f in rx.result()[0]]                     # (waits for all three)
    return frames, tuple(int(v) for v in rx.stats()[0])


def test_audio_loop(transmitted):
    audio, _, _ = transmitted
    frames, stats = receive(audio, len(audio))
    assert frames == fk.loop_packets()
    assert stats == (len(frames), 0, 0)


def _drain(blk, d_in, n_in, d_out, cap, in_es, out_es):
    """a stream block over a whole device window -> produced"""
    c_tot = p_tot = 0
    for _ in range(16):
        _, c, p, _ = blk.work_dev(d_in + c_tot * in_es, n_in - c_tot, d_out + p_tot * out_es, cap - p_tot)
        c_tot, p_tot = c_tot + c, p_tot + p
        if c_tot == n_in or (c == 0 and p == 0):
            break
    blk.sync()
    assert n_in - c_tot <= 1                   # (a block with history may keep the last sample for its next window)
    return p_tot


def test_rf_loop(transmitted):
    _, out, _ = transmitted
    no = len(out)
    t = fk.LOOP_TX
    demod = torch.zeros(no, dtype=torch.float32, device="cuda")
    back = torch.zeros(no // 4 + 8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # out = (sin p2, cos p2) = j e^(-j p2): a quadrature demodulator sees -k2 a, so its gain is -1 / k2
    nd = _drain(rr.QuadratureDemod(-1.0 / t["k2"]), out.data_ptr(), no, demod.data_ptr(), no, 8, 4)
    nb = _drain(rr.RationalResampler(1, 4, np.float32), demod.data_ptr(), nd, back.data_ptr(), len(back), 4, 4)
    assert no // 4 - 1 <= nb <= no // 4 + 1
    frames, stats = receive(back, nb)
    assert frames == fk.loop_packets()
    assert stats == (len(frames), 0, 0)
