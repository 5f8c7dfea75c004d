"""No GPU: the two statements of KissFrame -> KissDecode in tests/kiss_model.py against the reference's own vectors and against each
other, the encoder's model and the round trip, the arithmetic of rustradio_amd/csrc/kiss_core.hpp tile by tile on the CPU, the
host-only logic of rustradio_amd/csrc/kiss_host.hpp under the host sanitizers, and what rr.KissDecode / rr.KissEncode say without a
device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kiss_model as km
import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KA = km.known_answers()
BOTH = (km.SequentialDecoder, km.ClosedDecoder)


def test_constants_and_vector_counts():
    assert (km.FEND, km.FESC, km.TFEND, km.TFESC, km.MAX_LEN) == (0xC0, 0xDB, 0xDC, 0xDD, 10000) and KA["max_len"] == km.MAX_LEN
    assert rr.KISS_MAX_LEN == km.MAX_LEN
    assert len(KA["decode"]) == 1 and len(KA["encode"]) == 2 and len(KA["frame"]) == 3


@pytest.mark.parametrize("model", BOTH)
def test_decode_vectors_against_both_statements(model):
    for v in KA["decode"]:
        frame = bytes.fromhex(v["frame_hex"])              # KissDecode's input: strip_fend takes the leading FEND
        m = model()
        got = m.push(frame + bytes([km.FEND]))
        assert got == [(len(frame), v["port"], v["in_bytes"], bytes.fromhex(v["packet_hex"]))]
        assert len(got[0][3]) == v["out_bytes"] and m.stats() == (1, 1, 0, 0, 0)
        assert km.unescape(frame[2:]) == (bytes.fromhex(v["packet_hex"]), None)


@pytest.mark.parametrize("model", BOTH)
def test_frame_vectors_against_both_statements(model):
    for v in KA["frame"]:
        m = model()
        if "stream_hex" in v:
            got = m.push(bytes.fromhex(v["stream_hex"]))
            frames = [bytes.fromhex(f) for f in v["frames_hex"]]
            assert [(g[1], g[3]) for g in got] == [(f[0] >> 4, f[1:]) for f in frames] and m.stats()[0] == len(frames)
        else:
            data = bytes.fromhex(v["lead_hex"]) + bytes([v["fill"]]) * v["fill_count"] + bytes.fromhex(v["tail_hex"])
            assert m.push(data) == []                      # (the fill's first byte is a non-data port)
            assert m.stats() == (v["frames"], 0, v["frames"], 0, 1 - v["frames"])
            assert v["frame_len"] == (v["fill_count"] if v["frames"] else 0)


def test_encode_vectors():
    for v in KA["encode"]:
        p = bytes.fromhex(v["packet_hex"])
        out = km.encode_one(p, v["port"])
        assert out == bytes.fromhex(v["kiss_hex"]) and len(p) == v["in_bytes"] and len(out) == v["out_bytes"]
        assert km.encode_records([p], [v["port"]]) == [(0, v["out_bytes"], v["out_bytes"] - 3 - v["in_bytes"], v["port"])]


def _family():
    """(max_len, pushes) of the drawn family: heavy in the four special bytes, small max_len, 1 .. 5 pushes a stream"""
    rng = np.random.default_rng(2024)
    for it in range(6000):
        max_len = int(rng.choice([1, 2, 3, 5, 8, 10000], p=[0.05, 0.1, 0.15, 0.25, 0.25, 0.2]))
        n = int(rng.integers(1, 120))
        data = km.draw_stream(rng, n, special=float(rng.choice([0.25, 0.4, 0.55])))
        yield max_len, km.split(rng, data, int(rng.integers(1, 6)))


def test_the_two_statements_agree_on_a_drawn_family():
    """first, from the sequential model alone, that the family holds enough of every case; then that the closed form says the same
    packets push by push and the same counters"""
    fam = list(_family())
    tot = dict(delivered=0, empty=0, nondata=0, trailing=0, invalid=0, overlong=0, unsynced=0)
    seq = []
    for max_len, pushes in fam:
        m = km.SequentialDecoder(max_len)
        out, st = km.run(m, pushes)
        seq.append((out, st))
        tot["delivered"] += st[1]
        tot["empty"] += sum(1 for ps in out for p in ps if len(p[3]) == 0)
        tot["nondata"] += st[2]
        tot["trailing"] += m.bad_trailing
        tot["invalid"] += m.bad_invalid
        tot["overlong"] += st[4]
        tot["unsynced"] += b"".join(pushes)[:1] != bytes([km.FEND])
    print(tot)
    assert tot["delivered"] >= 1000 and tot["empty"] >= 100 and tot["nondata"] >= 100, tot
    assert tot["trailing"] >= 100 and tot["invalid"] >= 100 and tot["overlong"] >= 100 and tot["unsynced"] >= 100, tot
    for (max_len, pushes), (out, st) in zip(fam, seq):
        c = km.ClosedDecoder(max_len)
        assert km.run(c, pushes) == (out, st), (max_len, pushes)


def test_every_split_of_one_stream_into_two_pushes():
    rng = np.random.default_rng(10)
    data = bytes([km.FEND]) + km.draw_stream(rng, 300, special=0.5)
    for max_len in (8, 10000):
        whole, st = km.run(km.SequentialDecoder(max_len), [data])
        assert len(whole[0]) >= 5
        for cut in range(len(data) + 1):
            for model in BOTH:
                out, st2 = km.run(model(max_len), [data[:cut], data[cut:]])
                assert out[0] + out[1] == whole[0] and st2 == st, (max_len, cut, model)


def test_round_trip_and_the_port_12_quirk():
    rng = np.random.default_rng(8)
    packets = [b"", bytes([km.FEND]), bytes([km.FESC, km.TFEND]), km.draw_stream(rng, 40), bytes(rng.integers(0, 256, 100, dtype=np.uint8))]
    for port in range(16):
        stream = km.encode(packets, [port] * len(packets))
        for model in BOTH:
            got = model().push(stream)
            if port != 12:
                assert [(g[1], g[3]) for g in got] == [(port, p) for p in packets], port
            else:
                # the port byte 0xC0 is written raw (escape, :34): the decoder sees FEND FEND and takes the packet's first byte
                # as the port byte
                assert km.encode_one(b"\x00ab", 12) == bytes([km.FEND, km.FEND, 0, 0x61, 0x62, km.FEND])
                assert [(g[1], g[3]) for g in model().push(km.encode_one(b"\x00ab", 12))] == [(0, b"ab")]
                assert [(g[1], g[3]) for g in got] != [(port, p) for p in packets]
    assert km.encode_one(b"x", 16) == km.encode_one(b"x", 0) and km.encode_one(b"x", 99) == km.encode_one(b"x", 0)


def _build(src, exe, extra):
    subprocess.run(["g++", "-std=c++17", *extra, src, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_kiss_core_tile_by_tile_on_the_cpu(tmp_path):
    """tests/cpp/emu_kiss.cpp runs the kernels' arithmetic (kiss_core.hpp) thread by thread and tile by tile over streams this
    test draws, in the launch order of kernels_kiss.hip, and prints packets and counters; they are the model's"""
    exe = str(tmp_path / "emu_kiss")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "rustradio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "emu_kiss.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(9)
    for it in range(40):
        max_len = int(rng.choice([1, 3, 8, 40, 10000]))
        tile = int(rng.choice([16, 32, 64]))               # the emulation's tile: a multiple of the 16 bytes of a thread
        data = km.draw_stream(rng, int(rng.integers(1, 400)), special=float(rng.choice([0.2, 0.5])))
        pushes = km.split(rng, data, int(rng.integers(1, 5)))
        want, st = km.run(km.ClosedDecoder(max_len), pushes)
        text = f"{max_len} {tile} {len(pushes)}\n" + "".join(f"{len(p)} {p.hex() or '-'}\n" for p in pushes)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        got = [[] for _ in pushes]
        for ln in lines:
            f = ln.split()
            if f and f[0] == "P":
                got[int(f[1])].append((int(f[2]), int(f[3]), int(f[4]), bytes.fromhex(f[5]) if f[5] != "-" else b""))
        assert got == want, (max_len, tile, pushes)
        assert tuple(int(x) for x in [ln for ln in lines if ln.startswith("S ")][-1].split()[1:]) == st
    # the encoder's per-byte arithmetic
    enc = subprocess.run([exe, "encode"], input="c0dbdcdd00ff\n", capture_output=True, text=True, timeout=60)
    assert enc.returncode == 0 and enc.stdout.split() == ["1", "1", "0", "0", "0", "0", "ports", "0", "16", "192", "240", "0", "0"]


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """the plans, the refusals, the descriptors, the validation of hostile device numbers and the clamped copy-out as a stand-alone
    program built with -fsanitize=address,undefined (rustradio_amd/csrc/kiss_host.hpp compiles without HIP)"""
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    out = _build(os.path.join(ROOT, "tests", "cpp", "test_kiss_hostlogic.cpp"), str(tmp_path / "test_kiss_hostlogic"),
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("kiss host logic ok")


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "rustradio_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t, names = decl.rsplit(" ", 1)[0], decl
            t = re.match(r"(unsigned long long|unsigned|size_t)", decl).group(1)
            for n in decl[len(t):].split(","):
                fields.append((n.strip(), t))
    return fields


def test_symbols_and_record_layouts_match_the_header():
    from rustradio_amd._lib import SYMBOLS
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in ("rr_kiss_decode_create", "rr_kiss_decode_push_dev", "rr_kiss_decode_push", "rr_kiss_packets", "rr_kiss_packet_bytes",
              "rr_kiss_packet_bytes_dev", "rr_kiss_decode_stats", "rr_kiss_decode_dims", "rr_kiss_encode_create", "rr_kiss_encode_bound",
              "rr_kiss_encode_push_dev", "rr_kiss_encode_push", "rr_kiss_encode_records", "rr_kiss_encode_dims", "rr_kiss_encode_frames",
              "rr_hdlc_framer_push_kiss"):
        assert s in SYMBOLS and hasattr(L, s), s
    np_of = {"unsigned long long": np.uint64, "unsigned": np.uint32, "size_t": np.uintp}
    for name, dt, size in (("rr_kiss_packet", rr.KISS_PACKET, 32), ("rr_kiss_frame_record", rr.KISS_FRAME_RECORD, 24)):
        want = np.dtype([(n, np_of[t]) for n, t in _header_struct(name)], align=True)
        assert dt == want and dt.itemsize == size, (name, dt, want)
    assert rr.lib().rr_abi_version() == 3


def test_refusals_come_before_any_device():
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match=r"kiss decode: max_len out of range"):
            rr.KissDecode(bad)
    assert rr.KissEncode.bound([]) == 0 and rr.KissEncode.bound([0, 5, 1]) == 3 + 13 + 5
    assert rr.KissEncode.bound([2 ** 63, 2 ** 63]) == 2 ** 64 - 1      # saturates
    # not a handle at all: said by the ABI, nothing launched
    n0 = rr.lib().rr_debug_kernel_launches()
    assert rr.lib().rr_kiss_decode_push_dev(None, None, 4, None) != 0 and "not a kiss decode handle" in rr.last_error()
    assert rr.lib().rr_kiss_encode_dims(None, None, None) != 0 and "not a kiss encode handle" in rr.last_error()
    assert rr.lib().rr_debug_kernel_launches() == n0


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert rr.KissDecode().name == "KissFrame>KissDecode" and rr.KissEncode().name == "KissEncode>PduToStream"
    else:
        for make in (rr.KissDecode, rr.KissEncode):
            with pytest.raises(ValueError, match="no usable HIP device"):
                make()


def test_the_numpy_forms_the_probe_times():
    """encode_numpy and decode_numpy (tools/kiss_probe.py's host side) say what encode() and the decoders say"""
    rng = np.random.default_rng(12)
    for it in range(60):
        packets = [km.draw_stream(rng, int(rng.integers(0, 60)), special=0.4) for _ in range(int(rng.integers(1, 12)))]
        ports = [int(q) for q in rng.integers(0, 18, len(packets))]
        lens = np.array([len(p) for p in packets])
        arena = np.frombuffer(b"".join(packets) + b"\x00", np.uint8)
        assert km.encode_numpy(arena, np.cumsum(lens) - lens, lens, ports).tobytes() == km.encode(packets, ports)
        for max_len in (5, 10000):
            data = km.draw_stream(rng, int(rng.integers(1, 400)), special=float(rng.choice([0.2, 0.5])))
            want = km.ClosedDecoder(max_len).push(data)
            pos, port, inb, ln, arena = km.decode_numpy(np.frombuffer(data, np.uint8), max_len)
            at = np.cumsum(ln) - ln
            got = [(int(pos[i]), int(port[i]), int(inb[i]), arena[at[i]:at[i] + ln[i]].tobytes()) for i in range(len(pos))]
            assert got == want and len(arena) == int(ln.sum())
