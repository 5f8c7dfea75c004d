"""No GPU: the two statements of the transmit chain in tests/frame_model.py against the reference's own vectors and against each
other, a loop-back through the deframer's model, the arithmetic of rustradio_amd/csrc/frame_core.hpp on the CPU, the host-only
logic of the record path under the host sanitizers, and what rr.HdlcFramer says without a device."""
import json
import os
import subprocess

import numpy as np
import pytest

import bits_model as bm
import frame_model as fm
import hdlc_model as hm
import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "hdlc_framer_known_answers.json")))
FLAG = VECTORS["sync"] * VECTORS["sync_bytes"]


def test_vector_counts():
    assert len(VECTORS["various"]) == 7 and len(VECTORS["scrambler"]) == 2 and len(VECTORS["nrzi"]) == 2
    assert FLAG == fm.SYNC * fm.SYNC_BYTES and len(FLAG) == 160


@pytest.mark.parametrize("k", range(7))
def test_various_against_both_statements(k):
    v = VECTORS["various"][k]
    data = bytes.fromhex(v["bytes"])
    want = FLAG + [int(c) for c in v["bits"]] + FLAG
    got, recs = fm.FramerSeq(0).push([data])
    assert got.tolist() == want
    assert recs == [(0, len(want), len(v["bits"]) - 8 * len(data), 0)]
    got2, recs2 = fm.closed_form([data], 0)
    assert got2.tolist() == want and recs2 == recs


def test_fcs_vector_against_both_statements():
    data, app = bytes.fromhex(VECTORS["fcs"]["bytes"]), bytes.fromhex(VECTORS["fcs"]["appended"])
    assert fm.fcs_adder(data) == data + app
    assert fm.crc_by_division(data) == app[0] | app[1] << 8
    for packets in ([data], [b""], [b"\x00"], [b"\xff" * 40]):
        a, ra = fm.FramerSeq(fm.FCS).push(packets)
        b, rb = fm.closed_form(packets, fm.FCS)
        assert np.array_equal(a, b) and ra == rb
    assert fm.crc_by_division(b"") == hm.crc16_x25(b"") == 0


@pytest.mark.parametrize("k", range(2))
def test_scrambler_vectors_against_both_statements(k):
    v = VECTORS["scrambler"][k]
    line = v["input"] + [0] * v["flush"]
    seq = fm.FramerSeq(fm.G3RUH).line(line)
    assert seq[:v["skip"]] == [0] * 17                        # the register's zeros come out first
    assert seq[v["skip"]:] == v["scrambled"]
    assert fm.scramble_closed(np.array(line, np.uint8)).tolist() == seq
    assert bm.Lfsr(*bm.G3RUH).run(v["scrambled"]) == v["input"]          # and the receive side's Descrambler undoes it


def test_nrzi_vectors_against_both_statements():
    dec, enc = VECTORS["nrzi"]
    assert dec["block"] == "NrziDecode" and bm.Nrzi().run(dec["input"]) == dec["output"]
    assert enc["block"] == "NrziEncode"
    assert fm.FramerSeq(fm.NRZI).line(enc["input"]) == enc["output"]
    assert fm.nrzi_closed(np.array(enc["input"], np.uint8)).tolist() == enc["output"]
    assert bm.Nrzi().run(bm.nrzi_encode(dec["input"])) == dec["input"]


def test_the_two_statements_agree_on_5000_drawn_packets():
    """bytes drawn with P(bit = 1) = 0.9: stuffing is frequent; every flag combination; 1 .. 4 packets per stream"""
    rng = np.random.default_rng(21)
    done = stuffed = 0
    while done < 5000:
        flags = int(rng.integers(0, 16))
        packets = fm.draw_packets(rng, int(rng.integers(1, 5)), 24)
        a, ra = fm.FramerSeq(flags, -0.5, 2.0).push(packets)
        b, rb = fm.closed_form(packets, flags, -0.5, 2.0)
        assert a.dtype == b.dtype and np.array_equal(a, b), (flags, packets)
        assert ra == rb
        assert len(a) <= fm.bound(flags, [len(p) for p in packets])
        done += len(packets)
        stuffed += sum(r[2] for r in ra)
    assert stuffed > 5000


def test_the_bound_is_reached_by_all_ones():
    for flags in (0, fm.FCS):
        for n in (0, 1, 5, 64):
            p = b"\xff" * n
            out, recs = fm.closed_form([p], flags)
            if not flags:
                assert len(out) == fm.bound(flags, [n])
            assert len(out) <= fm.bound(flags, [n])


def test_the_split_into_pushes_does_not_change_the_stream():
    rng = np.random.default_rng(22)
    packets = fm.draw_packets(rng, 12, 30)
    for flags in (fm.G3RUH, fm.NRZI, fm.FCS | fm.G3RUH | fm.NRZI):
        whole, _ = fm.closed_form(packets, flags)
        m = fm.FramerSeq(flags)
        parts = [m.push(packets[i:j])[0] for i, j in ((0, 1), (1, 1), (1, 5), (5, 12))]
        assert np.array_equal(np.concatenate(parts), whole)


def test_loop_back_through_the_deframer_model():
    """framed bits of 1 .. 3 packets with the FCS go into HdlcModel, which returns every packet with a good CRC"""
    rng = np.random.default_rng(23)
    for it in range(60):
        packets = [p for p in fm.draw_packets(rng, int(rng.integers(1, 4)), 60, p_one=rng.choice([0.5, 0.9])) if len(p)]
        bits, _ = (fm.FramerSeq(fm.FCS).push(packets) if it & 1 else fm.closed_form(packets, fm.FCS))
        m = hm.HdlcModel(min_size=0, max_size=4096)
        got = [f[1] for f in m.run(bits)]
        assert got == packets, it
        assert m.stats() == (len(packets), 0, 0)
        # ... and through the line: the receive side's NrziDecode and Descrambler undo it, 17 bits late (the last 17 bits of the
        # closing flags still sit in the scrambler's register: 17 of 20 flags are left)
        line, _ = fm.closed_form(packets, fm.FCS | fm.G3RUH | fm.NRZI)
        dec = bm.Chain(nrzi=True, descrambler=bm.G3RUH, soft=False).run(line)[0]
        assert np.array_equal(dec[17:], bits[:-17])
        assert [f[1] for f in hm.HdlcModel(min_size=0, max_size=4096).run(dec[17:])] == packets


def _build(src, exe, extra):
    subprocess.run(["g++", "-std=c++17", *extra, src, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_frame_core_on_the_cpu(tmp_path):
    """the stuffing summary's combine, exhaustively up to 14 bits cut at every point, against the sequential counter; CRC chunks
    combined by x^(8 len); the tile recurrence c' = M c ^ z against the LFSR for 1,000 random tiles per mode"""
    out = _build(os.path.join(ROOT, "tests", "cpp", "emu_frame.cpp"), str(tmp_path / "emu_frame"),
                 ["-O2", "-I", os.path.join(ROOT, "rustradio_amd", "csrc")])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("frame core ok")


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """the bound, the refusals, the descriptors, the records and the clamped copy-out as a stand-alone program built with
    -fsanitize=address,undefined (rustradio_amd/csrc/frame_host.hpp compiles without HIP)"""
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    out = _build(os.path.join(ROOT, "tests", "cpp", "test_frame_hostlogic.cpp"), str(tmp_path / "test_frame_hostlogic"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("frame host logic ok")


def test_symbols_and_record_layout():
    import ctypes
    from rustradio_amd._lib import SYMBOLS
    for s in ("rr_nrzi_encode_create", "rr_scrambler_g3ruh_create", "rr_hdlc_framer_create", "rr_hdlc_framer_bound",
              "rr_hdlc_framer_push_dev", "rr_hdlc_framer_push", "rr_hdlc_framer_records", "rr_hdlc_framer_dims"):
        assert s in SYMBOLS and hasattr(ctypes.CDLL(rr.LIB_PATH), s)
    assert rr.FRAME_RECORD.itemsize == 24 and rr.FRAME_RECORD.fields["stuffed"][1] == 16 and rr.FRAME_RECORD.fields["fcs"][1] == 20
    assert (rr.FRAME_FCS, rr.FRAME_G3RUH, rr.FRAME_NRZI, rr.FRAME_SYMBOLS) == (fm.FCS, fm.G3RUH, fm.NRZI, fm.SYMBOLS)


def test_flag_error_comes_before_any_device():
    with pytest.raises(ValueError, match="unknown hdlc framer flags"):
        rr.HdlcFramer(16)
    with pytest.raises(ValueError, match="unknown hdlc framer flags"):
        rr.HdlcFramer(-1)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert rr.HdlcFramer(rr.FRAME_FCS).name != "" and rr.NrziEncode().name == "NrziEncode" and rr.Scrambler.g3ruh().name == "Scrambler"
    else:
        for make in (lambda: rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI), rr.NrziEncode, rr.Scrambler.g3ruh):
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()
