"""GPU: rr_kiss_decode and rr_kiss_encode (kernels_kiss.hip) against tests/kiss_model.py.  Every comparison is byte for byte: the
blocks are exact in integers, so there is no tolerance anywhere in this file.  Tile and carry come from the dims calls; every case
is a few pushes of at most about four tiles."""
import numpy as np
import pytest
import torch

import kiss_model as km
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
FEND, FESC, TFEND, TFESC = km.FEND, km.FESC, km.TFEND, km.TFESC
KA = km.known_answers()
SLACK = 257                           # canary bytes behind the bound


def launches():
    return rr.lib().rr_debug_kernel_launches()


def dev(data):
    data = bytes(data)
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda() if len(data) else torch.zeros(1, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def dims():
    T, carry, k = rr.KissDecode().dims()
    Te, ke = rr.KissEncode().dims()
    assert carry == km.MAX_LEN and T % 16 == 0 and Te % 16 == 0 and 1 <= k <= 7 and ke == 3
    return T, k, Te, ke


def decode_push(kd, data, host=False):
    """one push -> [(pos, port, in_bytes, bytes)]; the records are packed in stream order"""
    if host:
        got = kd.push(data)
    else:
        d = dev(data)
        kd.push_dev(d.data_ptr(), len(data))
        got = kd.result()
    rec = kd.packets()
    assert len(rec) == len(got) and np.all(rec["reserved"] == 0)
    assert np.array_equal(rec["start"], np.cumsum(rec["len"], dtype=np.uint64) - rec["len"]), "arena not packed in stream order"
    assert len(kd.packet_bytes()) == int(rec["len"].sum())
    return got


def check_decode(max_len, pushes, host=False):
    """a fresh handle and the closed-form model over the same pushes: packets push by push, counters behind every push"""
    kd, m = rr.KissDecode(max_len), km.ClosedDecoder(max_len)
    total = 0
    for p in pushes:
        want = m.push(p)
        got = decode_push(kd, p, host)
        assert got == want, (max_len, [len(q) for q in pushes])
        assert kd.stats() == m.stats()
        total += len(got)
    return total, m.stats()


def filler(n, seed=0):
    """n payload bytes with no special byte among them"""
    return bytes(0x20 + (i * 7 + seed) % 0x60 for i in range(n))


# ---- 1. the reference's vectors, through both ABIs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_vectors_through_both_abis(host):
    for v in KA["decode"]:
        frame = bytes.fromhex(v["frame_hex"])
        kd = rr.KissDecode()
        assert decode_push(kd, frame + bytes([FEND]), host) == [(len(frame), v["port"], v["in_bytes"], bytes.fromhex(v["packet_hex"]))]
        assert kd.stats() == (1, 1, 0, 0, 0)
    for v in KA["frame"]:
        kd = rr.KissDecode()
        if "stream_hex" in v:
            got = decode_push(kd, bytes.fromhex(v["stream_hex"]), host)
            assert [bytes([g[1] << 4]) + g[3] for g in got] == [bytes.fromhex(f) for f in v["frames_hex"]]
        else:
            data = bytes.fromhex(v["lead_hex"]) + bytes([v["fill"]]) * v["fill_count"] + bytes.fromhex(v["tail_hex"])
            assert decode_push(kd, data, host) == []
            assert kd.stats() == (v["frames"], 0, v["frames"], 0, 1 - v["frames"])
            # the same gap with a data port in front: delivered at exactly MAX_LEN, dropped one byte beyond
            kd2 = rr.KissDecode()
            got = decode_push(kd2, data[:1] + b"\x00" + data[2:], host)
            assert [len(g[3]) for g in got] == ([v["fill_count"] - 1] if v["frames"] else [])
    ke = rr.KissEncode()
    for v in KA["encode"]:
        p = bytes.fromhex(v["packet_hex"])
        if host:
            out = ke.push([p], [v["port"]])
        else:
            out, _ = encode_dev(ke, [p], [v["port"]])
        assert out == bytes.fromhex(v["kiss_hex"])
        rec, produced = ke.records()
        assert produced == v["out_bytes"] and int(rec[0]["len"]) == v["out_bytes"] and int(rec[0]["port"]) == v["port"]


# ---- 2. decode: seams ------------------------------------------------------------------------------------------------------------------
def seam_streams(T):
    """name -> (max_len, pushes)"""
    out = {}
    s = bytearray(filler(2 * T + 10))
    s[0], s[1], s[T - 1], s[T], s[T + 1], s[T + 5] = FEND, 0x00, FEND, FEND, 0x10, FEND
    out["fend last of a tile and first of the next"] = (10000, [bytes(s)])
    for name, nxt in (("tfend", TFEND), ("tfesc", TFESC), ("wrong byte", 0x41), ("fesc", FESC), ("fend", FEND)):
        s = bytearray(filler(T + 40, 3))
        s[0], s[1], s[T - 1], s[T], s[T + 30] = FEND, 0x20, FESC, nxt, FEND
        out[f"fesc last of a tile, {name} first of the next"] = (10000, [bytes(s)])
        out[f"fesc last of a push, {name} first of the next"] = (10000, [bytes(s[:T]), bytes(s[T:])])
        out[f"fesc last of a short push, {name} first of the next"] = (10000, [bytes(s[:7] + bytes([FESC])), bytes([nxt]) + bytes(s[9:20]) + bytes([FEND])])
    g = bytes([FEND, 0x30]) + filler(2 * T + T // 2) + bytes([FESC, TFEND, FEND])
    out["a gap spanning three tiles"] = (3 * T, [filler(T // 2) + g])
    out["a gap spanning three tiles in three pushes"] = (3 * T, [filler(5) + g[:T], g[T:2 * T + 1], g[2 * T + 1:]])
    M = T + 3
    for extra in (0, 1):
        g = bytes([FEND, 0x00]) + filler(M - 1 + extra, 5) + bytes([FEND, 0x10, 0x31, FEND])
        name = "max_len" if extra == 0 else "max_len + 1"
        out[f"a gap of {name} inside one push"] = (M, [g])
        out[f"a gap of {name} across a push"] = (M, [g[:100], g[100:]])
        out[f"a gap of {name} in three pushes, the last one the closing fend"] = (M, [g[:T], g[T:M + 1 + extra], g[M + 1 + extra:]])
    out["only fends"] = (10000, [bytes([FEND]) * (3 * T + 5)])
    out["only fends in two pushes"] = (10000, [bytes([FEND]) * T, bytes([FEND]) * (T + 1)])
    out["only fescs"] = (10000, [bytes([FESC]) * (2 * T + 5)])
    out["only fescs behind a fend"] = (10000, [bytes([FEND, 0x00]) + bytes([FESC]) * (T + 5) + bytes([FEND])])
    out["no fend at all, then a push that syncs"] = (10000, [filler(T + 9), filler(30), bytes([0x00, FEND, 0x00, 0x41, FEND])])
    out["no fend for longer than max_len, then a push that syncs"] = (5, [filler(40), bytes([0x00, FEND, 0x00, 0x41, FEND])])
    out["an open gap that outgrows max_len between pushes"] = (5, [bytes([FEND, 0x00, 0x41]), filler(2), filler(2), bytes([FEND, 0x00, FEND])])
    out["empty packets in every even slot of a tile"] = (10000, [bytes([FEND, 0x00]) * (T + 8)])
    out["empty packets in every odd slot of a tile"] = (10000, [bytes([0x00, FEND]) * (T + 8)])
    out["empty packets with max_len 1"] = (1, [bytes([FEND, 0x00]) * 40 + bytes([FEND, 0x00, 0x00, FEND, 0x10, FEND])])
    ports = b"".join(bytes([FEND, p]) + filler(3, p) for p in list(range(1, 16)) + [FESC, TFEND, 0xFF, 0x00, 0xF0])
    out["non-data ports"] = (10000, [ports + bytes([FEND])])
    return out


def test_decode_seams(dims):
    T = dims[0]
    cases = seam_streams(T)
    delivered = 0
    for name, (max_len, pushes) in cases.items():
        kd, m = rr.KissDecode(max_len), km.ClosedDecoder(max_len)
        for p in pushes:
            want = m.push(p)
            assert decode_push(kd, p) == want, name
            assert kd.stats() == m.stats(), name
            delivered += len(want)
    assert delivered > 2 * T            # (the cases do deliver: the empty packets alone are 2 T)
    # what the cases are there for, from the model alone
    def stats(name):
        max_len, pushes = cases[name]
        return km.run(km.SequentialDecoder(max_len), pushes)[1]
    assert stats("a gap of max_len inside one push") == (2, 2, 0, 0, 0) and stats("a gap of max_len + 1 across a push") == (1, 1, 0, 0, 1)
    assert stats("fesc last of a push, tfend first of the next") == (1, 1, 0, 0, 0)
    assert stats("fesc last of a push, wrong byte first of the next") == (1, 0, 0, 1, 0)
    assert stats("non-data ports") == (20, 2, 18, 0, 0) and stats("a gap spanning three tiles in three pushes") == (1, 1, 0, 0, 0)
    assert stats("no fend for longer than max_len, then a push that syncs") == (1, 1, 0, 0, 0)
    assert stats("an open gap that outgrows max_len between pushes") == (1, 1, 0, 0, 1)


# ---- 3. decode: fuzz -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(10))
def test_decode_fuzz(dims, seed):
    """20 streams a seed (200 in all) of up to 3 T bytes in 1 .. 4 pushes: packets, records, pos, the counters and the packed arena"""
    T = dims[0]
    rng = np.random.default_rng(500 + seed)
    total = 0
    for it in range(20):
        max_len = int(rng.choice([1, 3, 8, 100, T + 3, 10000]))
        n = int(rng.integers(1, 3 * T + 1)) if it % 4 else int(rng.integers(1, 64))
        data = km.draw_stream(rng, n, special=float(rng.choice([0.02, 0.1, 0.4])))
        total += check_decode(max_len, km.split(rng, data, int(rng.integers(1, 5))), host=it % 5 == 0)[0]
    assert total > 50


# ---- 4. encode -------------------------------------------------------------------------------------------------------------------------
def encode_dev(ke, packets, ports=None, geom=None):
    """one push through device buffers -> (bytes, records); the bytes behind `produced` keep their canary"""
    if geom is None:
        lens = np.array([len(p) for p in packets], np.uintp)
        data, starts = b"".join(bytes(p) for p in packets), (np.cumsum(lens) - lens).astype(np.uintp)
    else:
        data, starts, lens = geom
    d_in = dev(data)
    cap = rr.KissEncode.bound(lens)
    d_out = torch.full((cap + SLACK,), 0xA5, dtype=torch.uint8, device="cuda")
    ke.push_dev(d_in.data_ptr(), len(data), starts, lens, ports, d_out.data_ptr(), cap)
    rec, produced = ke.records()
    out = d_out.cpu().numpy()
    assert produced <= cap and np.all(out[produced:] == 0xA5), "bytes at and beyond `produced` were written"
    return out[:produced].tobytes(), rec


def check_encode(ke, packets, ports=None):
    out, rec = encode_dev(ke, packets, ports)
    assert out == km.encode(packets, ports)
    want = km.encode_records(packets, ports)
    assert [(int(r["start"]), int(r["len"]), int(r["escaped"]), int(r["port"])) for r in rec] == want
    return out


def test_encode_cases(dims):
    Te = dims[2]
    ke = rr.KissEncode()
    rng = np.random.default_rng(31)
    check_encode(ke, [b""])
    check_encode(ke, [b"", b"", b""], [1, 2, 3])
    check_encode(ke, [b"", b"a", b"", b"", filler(Te), b""])
    only = bytes([FEND]) * (Te + 7)
    assert len(check_encode(ke, [only])) == rr.KissEncode.bound([len(only)])          # reaches the bound
    check_encode(ke, [bytes([FESC]) * 33, bytes([FEND, FESC]) * 50])
    # packet boundaries on and around a tile seam
    for a in (Te - 1, Te, Te + 1):
        check_encode(ke, [filler(a), bytes([FEND, FESC, 0x41]), filler(Te - 3), b"", bytes([FESC])], [0, 1, 2, 3, 4])
    # escapes on both sides of a seam
    p = bytearray(filler(2 * Te))
    p[Te - 1], p[Te] = FEND, FESC
    check_encode(ke, [bytes(p)])
    # ports 0, 12, 15, 16 and beyond: 12 writes a raw 0xC0, 16 and more are 0
    out = check_encode(ke, [b"ab", b"cd", b"ef", b"gh", b"ij"], [0, 12, 15, 16, 4000000000])
    assert out[5:7] == bytes([FEND, FEND]) and out[11] == 0xF0 and out[16] == 0x00 and out[21] == 0x00
    # drawn batches, several tiles
    for it in range(6):
        packets = [km.draw_stream(rng, int(rng.integers(0, 700)), special=float(rng.choice([0.0, 0.3, 0.9]))) for _ in range(int(rng.integers(1, 30)))]
        check_encode(ke, packets, [int(q) for q in rng.integers(0, 18, len(packets))])
    # overlapping and repeated input ranges
    data = km.draw_stream(rng, 300, special=0.4)
    starts, lens = np.array([0, 0, 10, 5, 299, 300, 100], np.uintp), np.array([300, 300, 50, 200, 1, 0, 0], np.uintp)
    out, rec = encode_dev(ke, None, None, geom=(data, starts, lens))
    assert out == km.encode([data[int(s):int(s) + int(n)] for s, n in zip(starts, lens)])
    # the round trip through the device decoder, port 12 apart
    packets = [km.draw_stream(rng, int(rng.integers(0, 300)), special=0.5) for _ in range(40)]
    ports = [int(q) for q in rng.integers(0, 12, len(packets))]
    kd = rr.KissDecode()
    assert [(g[1], g[3]) for g in decode_push(kd, check_encode(ke, packets, ports))] == list(zip(ports, packets))


# ---- 5. launches and refusals ---------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_the_contents(dims):
    T, k, Te, kenc = dims
    rng = np.random.default_rng(41)
    n = 2 * T + 100
    kd, ke = rr.KissDecode(), rr.KissEncode()
    for data in (bytes([FEND]) * n, bytes([FESC]) * n, bytes(n), bytes(rng.integers(0, 256, n, dtype=np.uint8)), bytes([FEND]), b"\x00"):
        d = dev(data)
        n0 = launches()
        kd.push_dev(d.data_ptr(), len(data))
        assert launches() - n0 == k
        kd.packets()
        assert launches() - n0 == k      # the read-back launches nothing
        lens = np.array([len(data) // 2, len(data) - len(data) // 2], np.uintp)
        starts = np.array([0, len(data) // 2], np.uintp)
        cap = rr.KissEncode.bound(lens)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n0 = launches()
        ke.push_dev(d.data_ptr(), len(data), starts, lens, None, d_out.data_ptr(), cap)
        assert launches() - n0 == kenc
        assert ke.records()[1] == len(km.encode([data[:len(data) // 2], data[len(data) // 2:]])) and launches() - n0 == kenc


def test_empty_pushes_and_refusals_launch_nothing(dims):
    kd, ke = rr.KissDecode(8), rr.KissEncode()
    m = km.ClosedDecoder(8)
    first = bytes([FEND, 0x00, 0x41, 0x42])
    assert decode_push(kd, first) == m.push(first)
    d = dev(b"abcd")
    d_out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    n0 = launches()
    kd.push_dev(d.data_ptr(), 0)
    kd.push_dev(0, 0)
    assert kd.result() == [] and kd.push(b"") == []
    for args, msg in (((0, 4), "kiss decode: null input"), ((d.data_ptr(), (1 << 30) + 1), "kiss decode: more than 2\\^30 bytes")):
        with pytest.raises(ValueError, match=msg):
            kd.push_dev(*args)
    ke.push_dev(d.data_ptr(), 4, [], [], None, d_out.data_ptr(), 0)
    assert ke.records()[1] == 0 and len(ke.records()[0]) == 0 and ke.push([]) == b""
    bound = rr.KissEncode.bound([4, 2])
    for args, msg in (((d.data_ptr(), 4, [0, 1], [4, 2], None, d_out.data_ptr(), bound - 1), "kiss encode: output shorter"),
                      ((d.data_ptr(), 4, [0, 3], [4, 2], None, d_out.data_ptr(), bound), "kiss encode: packet outside the buffer"),
                      ((d.data_ptr(), 4, [5], [0], None, d_out.data_ptr(), bound), "kiss encode: packet outside the buffer"),
                      ((0, 4, [0], [4], None, d_out.data_ptr(), bound), "kiss encode: null argument"),
                      ((d.data_ptr(), 4, [0], [4], None, 0, bound), "kiss encode: null argument"),
                      ((d.data_ptr(), (1 << 30) + 1, [0], [4], None, d_out.data_ptr(), bound), "kiss encode: more than 2\\^30 bytes"),
                      ((d.data_ptr(), 1 << 30, [0, 0, 0], [1 << 29] * 3, None, d_out.data_ptr(), 1 << 40), "kiss encode: more than 2\\^30 encoded bytes")):
        with pytest.raises(ValueError, match=msg):
            ke.push_dev(*args)
    assert launches() == n0
    assert np.all(d_out.cpu().numpy() == 0xA5)
    with pytest.raises(RuntimeError, match="KissDecode delivers packets"):      # rr_block_work: batch blocks have no stream protocol
        kd.work(np.zeros(4, np.uint8), 4)
    with pytest.raises(RuntimeError, match="KissEncode takes whole packets"):
        ke.work(np.zeros(4, np.uint8), 4)
    # the refusals and the pushes of nothing left every state alone: the open gap is closed by the next push
    rest = bytes([0x43, FEND])
    assert decode_push(kd, rest) == m.push(rest) == [(5, 0, 3, b"ABC")]
    assert kd.stats() == m.stats() == (1, 1, 0, 0, 0)
