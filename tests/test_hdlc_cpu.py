"""CPU: the two formulations of HdlcDeframer in tests/hdlc_model.py — the reference's sequential machine and the data-parallel
flag-to-flag event formulation — against the reference's own vectors and against each other."""
import json
import os

import numpy as np
import pytest

import hdlc_model as hm
from hdlc_model import FLAG, HdlcModel, bytes_to_bits, crc16_x25, deframe_events, frame_bits, stuff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "hdlc_known_answers.json")))


def both(bits, cfg):
    """(frames, stats) of the two formulations, which must agree"""
    m = HdlcModel(*cfg)
    seq = (m.run(bits), m.stats())
    assert deframe_events(bits, *cfg) == seq, cfg
    return seq


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_model_reproduces_the_reference_vectors(case):
    cfg = (case["min_size"], case["max_size"], case["keep_checksum"], False)
    for s in case["bits"]:
        bits = [int(c) for c in s]
        frames, _ = both(bits, cfg)
        assert [f[1] for f in frames] == [bytes(f) for f in case["frames"]]
        # one bit per run() call: the state is carried
        m = HdlcModel(*cfg)
        assert sum((m.run([b]) for b in bits), []) == frames


def test_crc_bitfix_vector():
    g = GOLDEN["crc_bitfix"]
    data = bytes(g["data"])
    good = crc16_x25(data)
    new, crc, fixed = hm.find_right_crc(data, good ^ (1 << g["flipped_crc_bit"]), True)
    assert fixed is g["fixed"] and new is g["new_data"] and crc == good


def test_crc_check_value():
    assert crc16_x25(b"123456789") == 0x906E
    assert crc16_x25(b"") == 0


def test_event_formulation_equals_the_sequential_machine():
    rng = np.random.default_rng(2024)
    frames_seen = 0
    for _ in range(5000):
        bits = hm.draw_stream(rng, int(rng.integers(1, 400)))
        cfg = (int(rng.integers(0, 4)), int(rng.integers(0, 11)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        frames_seen += len(both(bits, cfg)[0])
    assert frames_seen > 2000


def test_split_into_calls_does_not_matter():
    rng = np.random.default_rng(7)
    bits = hm.draw_stream(rng, 3000)
    whole = HdlcModel(1, 10).run(bits)
    m, got = HdlcModel(1, 10), []
    for a in range(0, 3000, 37):
        got += m.run(bits[a:a + 37])
    assert got == whole and len(whole) > 5


# ---- the quirks, each by name ----------------------------------------------------------------------------------------------------
def test_a_frame_of_exactly_max_size_bytes_is_dropped():
    for max_size in (3, 10):
        for nbytes, delivered in ((max_size - 1, True), (max_size, False)):
            payload = bytes(range(1, nbytes + 1))
            frames, _ = both(frame_bits(payload, with_crc=False), (1, max_size, True, False))
            assert [f[1] for f in frames] == ([payload] if delivered else [])


def test_after_two_flags_sharing_a_zero_a_third_sharing_again_stays_unsynced():
    body = stuff(bytes_to_bits(b"\x42")) + FLAG
    shared = lambda k: FLAG[:7] * k + [0]
    # two flags sharing their zero: fewer than 7 bits were collected, the machine resets AT the second flag, and a third flag sharing
    # again (7 bits later) is not seen; the fourth is, as a plain first flag
    found = {k: [f[1] for f in both(shared(k) + body, (1, 10, True, False))[0]] for k in (1, 2, 3, 4, 5)}
    assert found == {1: [b"\x42"], 2: [], 3: [], 4: [b"\x42"], 5: []}


def test_an_overlong_reset_inside_the_last_7_bits_hides_the_flag():
    behind = stuff(bytes_to_bits(b"\x15")) + FLAG
    for max_size in (3, 10):
        for extra, hidden in ((-7, False), (-6, False), (-5, True), (1, True), (2, False)):
            # the reset comes extra + 6 bits before the closing flag's end (hdlc_deframer.rs:144-146 runs before the bit is looked at)
            bits = FLAG + [0] * (8 * max_size + extra) + FLAG + behind
            frames, _ = both(bits, (1, max_size, True, False))
            assert (b"\x15" not in [f[1] for f in frames]) == hidden, (max_size, extra)


def test_a_flip_in_the_crc_field_raises_both_counters_and_emits_nothing():
    payload = b"hello, world"
    c = crc16_x25(payload) ^ 0x0400
    bits = FLAG + stuff(bytes_to_bits(payload + bytes([c & 0xff, c >> 8]))) + FLAG
    assert both(bits, (1, 100, False, True)) == ([], (0, 1, 1))
    assert both(bits, (1, 100, False, False)) == ([], (0, 1, 0))


def test_an_empty_frame_is_emitted_with_min_size_0_and_keep_checksum():
    bits = FLAG + FLAG
    assert both(bits, (0, 10, True, False)) == ([(15, b"", False)], (1, 0, 0))
    assert both(bits, (0, 10, False, False)) == ([], (0, 0, 0))          # fewer than 2 bytes: nothing, no counter
    assert both(bits, (1, 10, True, False)) == ([], (0, 0, 0))


def test_single_bit_repair_takes_the_lowest_byte_and_bit():
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
    raw = bytes_to_bits(payload + bytes([crc16_x25(payload) & 0xff, crc16_x25(payload) >> 8]))
    for k in (0, 77, 8 * 24 - 1):
        broken = list(raw)
        broken[k] ^= 1
        bits = FLAG + stuff(broken) + FLAG
        assert both(bits, (1, 100, False, True)) == ([(len(bits) - 1, payload, True)], (1, 0, 1))
        assert both(bits, (1, 100, False, False)) == ([], (0, 1, 0))


# ---- find_right_crc_lockstep, the repair of the long bodies ---------------------------------------------------------------------------
def test_lockstep_repair_equals_find_right_crc():
    rng = np.random.default_rng(31)
    assert hm.find_right_crc_lockstep(b"", 0x1234, True) == hm.find_right_crc(b"", 0x1234, True)
    assert hm.find_right_crc_lockstep(b"", 0x0001, True) == hm.find_right_crc(b"", 0x0001, True) == (None, 0x0000, True)
    seen = set()
    for n in (1, 2, 24, 100):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        good = crc16_x25(data)
        cases = [(data, good, "intact")]
        for h in sorted({0, 1, 7, 8 * n // 2, 8 * n - 8, 8 * n - 1} & set(range(8 * n))):
            broken = bytearray(data)
            broken[h >> 3] ^= 1 << (h & 7)
            cases.append((bytes(broken), good, "data"))
        cases += [(data, good ^ (1 << c), "crc") for c in range(16)]
        cases += [(data, good ^ 0x0003, "two crc bits"), (data, good ^ 0x8001, "two crc bits")]
        for body, got, what in cases:
            for fix in (False, True):
                want = hm.find_right_crc(body, got, fix)
                assert hm.find_right_crc_lockstep(body, got, fix) == want, (n, what, fix)
                seen.add((what, fix, want[0] is not None, want[2]))
    # a repaired body, a repaired checksum, nothing to repair and nothing repairable have all been seen (two wrong CRC bits look
    # like one wrong data bit for some bodies, so "two crc bits" may be either of the last two)
    assert ("data", True, True, True) in seen and ("crc", True, False, True) in seen and ("intact", True, False, False) in seen
    assert any(s[0] == "two crc bits" and s[1] and not s[3] for s in seen)
    assert all(not s[3] for s in seen if not s[1])


def test_lockstep_repair_past_the_crc_period():
    """CRC-16/X.25 has period 32,767: in a body of 4,200 bytes bit h and bit h + 32,767 change the CRC alike, and so do CRC-field
    bit c and data bit 833 + c.  find_right_crc takes the lowest, whatever was flipped (hdlc_deframer.rs:41-71)."""
    rng = np.random.default_rng(32)
    data = rng.integers(0, 256, 4200, dtype=np.uint8).tobytes()
    good = crc16_x25(data)

    def flipped(h):
        b = bytearray(data)
        b[h >> 3] ^= 1 << (h & 7)
        return bytes(b)

    def repaired_bit(new, old):
        d = np.flatnonzero(np.unpackbits(np.frombuffer(new, np.uint8) ^ np.frombuffer(old, np.uint8), bitorder="little"))
        assert len(d) == 1
        return int(d[0])

    for h, lowest in ((32767, 0), (33599, 832)):
        new, crc, fixed = hm.find_right_crc_lockstep(flipped(h), good, True)
        assert fixed and crc == good and repaired_bit(new, flipped(h)) == lowest
    for c in (0, 7, 8, 15):
        new, crc, fixed = hm.find_right_crc_lockstep(data, good ^ (1 << c), True)
        assert fixed and crc == good ^ (1 << c) and repaired_bit(new, data) == 833 + c          # a corrupt frame is delivered
        assert crc16_x25(new) == crc
    # HdlcModel with it in find_right_crc's place: the frame comes out with bit 0 turned over as well
    bits = FLAG + stuff(bytes_to_bits(flipped(32767) + bytes([good & 0xff, good >> 8]))) + FLAG
    m = HdlcModel(0, 65535, False, True, hm.find_right_crc_lockstep)
    assert m.run(bits) == [(len(bits) - 1, flipped(0)[:4095] + flipped(32767)[4095:], True)] and m.stats() == (1, 0, 1)
