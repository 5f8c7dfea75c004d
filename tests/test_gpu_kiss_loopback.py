"""GPU: the host side of examples/bell202.rs / examples/g3ruh.rs with the payload bytes on the device from end to end:
a KISS byte stream -> rr.KissDecode -> rr.HdlcFramer.push_kiss (FCS | NRZI, as levels) -> rr.BitDecoder (NRZI) ->
rr.HdlcDeframer(10, 1500) -> rr.KissEncode.encode_frames, and the same for three streams through rr.HdlcReceiver with a
port_of_stream table.  The result is the model's re-encoding of what the models of the blocks in between deliver, byte for byte."""
import numpy as np
import pytest
import torch

import bits_model as bm
import frame_model as fm
import hdlc_model as hm
import kiss_model as km
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
MIN_SIZE, MAX_SIZE = 10, 1500


def kiss_stream(rng, npackets):
    """a KISS stream of packets of 0 .. 80 bytes (many below min_size once the FCS is on) with noise between the frames:
    non-data frames, bad escapes, repeated FENDs, bytes in front of the first FEND"""
    parts = [bytes(rng.integers(0, 0xC0, 5, dtype=np.uint8))]
    for i in range(npackets):
        n = int(rng.integers(0, 14)) if i % 3 == 0 else int(rng.integers(14, 81))
        parts.append(km.encode_one(km.draw_stream(rng, n, special=0.3), int(rng.integers(0, 12))))
        k = int(rng.integers(0, 5))
        if k == 0:
            parts.append(bytes([0x06, 0x01, 0x02, km.FEND]))                   # a non-data frame
        elif k == 1:
            parts.append(bytes([0x00, 0x41, km.FESC, 0x42, km.FEND]))          # a bad escape
        elif k == 2:
            parts.append(bytes([km.FEND]) * int(rng.integers(1, 4)))
    return b"".join(parts)


def model_frames(packets):
    """what HdlcDeframer(MIN_SIZE, MAX_SIZE) delivers of the framed packets: the blocks' models in a row"""
    line, _ = fm.closed_form(packets, fm.FCS | fm.NRZI)
    bits = bm.Nrzi().run(line.tolist())
    return [f[1] for f in hm.HdlcModel(MIN_SIZE, MAX_SIZE).run(bits)]


def transmit(kd, fr, data, d_sym_ptr, cap):
    """KissDecode -> HdlcFramer.push_kiss on the device -> (the packets the model says, the levels produced)"""
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    kd.push_dev(d.data_ptr(), len(data))
    assert fr.bound(kd.packets()["len"]) <= cap
    fr.push_kiss(kd, d_sym_ptr, cap)
    return fr.records()[1]


def test_one_stream_through_the_deframer():
    rng = np.random.default_rng(61)
    data = kiss_stream(rng, 40)
    packets = [p[3] for p in km.ClosedDecoder().push(data)]
    want = model_frames(packets)
    assert len(packets) == 40 and 15 <= len(want) < len(packets)               # short packets fall out at min_size
    assert sorted(want) == sorted(p for p in packets if len(p) + 2 >= MIN_SIZE)
    kd, fr = rr.KissDecode(), rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
    rx, df, ke = rr.BitDecoder(nrzi=True), rr.HdlcDeframer(MIN_SIZE, MAX_SIZE), rr.KissEncode()
    cap = fm.bound(fm.FCS, [len(p) for p in packets])
    d_sym = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = transmit(kd, fr, data, d_sym.data_ptr(), cap)
    assert n == len(fm.closed_form(packets, fm.FCS)[0])
    assert rx.work_dev(d_sym.data_ptr(), n, d_bits.data_ptr(), n)[1:3] == (n, n)
    df.push_dev(d_bits.data_ptr(), n)
    out_cap = rr.KissEncode.bound(df.frames()["len"])
    d_out = torch.full((out_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ke.encode_frames(df, d_out.data_ptr(), out_cap)
    rec, produced = ke.records()
    out = d_out.cpu().numpy()
    assert out[:produced].tobytes() == km.encode(want) and np.all(out[produced:] == 0xA5)
    assert [(int(r["start"]), int(r["len"]), int(r["escaped"]), int(r["port"])) for r in rec] == km.encode_records(want)
    # ... which the decoder takes back
    assert [p[3] for p in rr.KissDecode().push(out[:produced].tobytes())] == want
    # any other handle is refused, and one too short a buffer, with nothing launched
    n0 = rr.lib().rr_debug_kernel_launches()
    with pytest.raises(ValueError, match="not an hdlc deframer or receiver handle"):
        ke.encode_frames(kd, d_out.data_ptr(), out_cap)
    with pytest.raises(ValueError, match="kiss encode: output shorter"):
        ke.encode_frames(df, d_out.data_ptr(), out_cap - 1)
    with pytest.raises(RuntimeError, match="not a kiss decode handle"):
        fr.push_kiss(df, d_sym.data_ptr(), cap)
    assert rr.lib().rr_debug_kernel_launches() == n0


def test_three_streams_through_the_receiver():
    rng = np.random.default_rng(62)
    N, table = 3, [5, 12, 0]
    datas = [kiss_stream(rng, 12 + 4 * c) for c in range(N)]
    packets = [[p[3] for p in km.ClosedDecoder().push(d)] for d in datas]
    want = [model_frames(p) for p in packets]
    assert all(0 < len(w) < len(p) for w, p in zip(want, packets))
    stride = max(fm.bound(fm.FCS, [len(p) for p in ps]) for ps in packets)
    d_sym = torch.zeros((N, stride), dtype=torch.float32, device="cuda")
    counts = []
    for c in range(N):
        kd, fr = rr.KissDecode(), rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
        counts.append(transmit(kd, fr, datas[c], d_sym.data_ptr() + 4 * c * stride, stride))
    d_counts = torch.from_numpy(np.asarray(counts, np.int64)).cuda()
    rx, ke = rr.HdlcReceiver(N, MIN_SIZE, MAX_SIZE, nrzi=True), rr.KissEncode()
    rx.push_dev(d_sym.data_ptr(), stride, stride, d_counts.data_ptr())
    assert [[f[1] for f in s] for s in rx.result()] == want
    out_cap = rr.KissEncode.bound(rx.frames()["len"])
    d_out = torch.full((out_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="kiss encode: port_of_stream shorter"):
        ke.encode_frames(rx, d_out.data_ptr(), out_cap, table[:2])
    ke.encode_frames(rx, d_out.data_ptr(), out_cap, table)
    produced = ke.records()[1]
    flat = [f for s in want for f in s]
    ports = [table[c] for c in range(N) for _ in want[c]]
    out = d_out.cpu().numpy()
    assert out[:produced].tobytes() == km.encode(flat, ports) and np.all(out[produced:] == 0xA5)
