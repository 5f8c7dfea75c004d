"""GPU: rr.Il2pReceiver against tests/il2p_model.py, the reference's blocks line by line, on the same bits: records, stats and
positions, whatever the split into pushes, the tiles, the other streams and the counts on the device.  Symbols are +-1.0 from bits
unless stated.  tests/test_il2p_cpu.py shows on the models that the fuzz cases and the loop-back line are not empty."""
import numpy as np
import pytest
import torch

import afsk_model as am
import fsk_model as fk
import il2p_cases as ic
import il2p_model as im
import rustradio_amd as rr

pytestmark = pytest.mark.gpu


def run_device(rx, streams, pushes, invert=False):
    """the pushes through rr_il2p_receiver_push -> [records of push k]"""
    return [ic.device_records(rx.push(a, counts)) for a, (_, counts) in zip(ic.host_rows(streams, pushes, invert), pushes)]


def check(streams, pushes, allowed=0, invert=False, rx=None):
    """device == model, push by push; -> the model's (per_push, stats)"""
    streams = [np.asarray(s, np.uint8) for s in streams]
    rx = rx or rr.Il2pReceiver(len(streams), invert=invert, allowed_diffs=allowed)
    want, stats, consumed = ic.expected(streams, pushes, allowed)
    got = run_device(rx, streams, pushes, invert)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, pushes[k], g, w)
    assert [tuple(int(v) for v in row) for row in rx.stats()] == stats
    assert rx.consumed().tolist() == consumed
    return want, stats


def noise(n, seed, allowed=0):
    """random bits in which nothing is within allowed_diffs of the sync word: the first seed from `seed` on that gives such"""
    while True:
        b = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)
        if not im.run(b, allowed)[1]:
            return b
        seed += 1000


def plant(bits, at, fb):
    bits[at:at + len(fb)] = fb
    return bits


# ---- 1. the reference's own vector ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, 1, 23, 24, 120, 121, 500])
def test_golden_bits(size):
    """one header, with the reference's values, in the push that holds position 905 and in no other"""
    bits = im.golden_bits()
    pushes = ic.even_pushes([bits], len(bits) if size is None else size)
    rx = rr.Il2pReceiver(1)
    got = run_device(rx, [bits], pushes)
    g = im.GOLDEN
    at = 0
    for (n, _), recs in zip(pushes, got):
        if at <= 905 < at + n:
            assert recs == [(0, 785, 0, g["raw"], "2E0QQQ", 1, "M0THC", 1, 2 | 4, 1, 0x44, 0)]
        else:
            assert recs == []
        at += n
    assert rx.stats().tolist() == [[1, 1]] and rx.consumed().tolist() == [1177]
    check([bits], pushes)


# ---- 2. push seams --------------------------------------------------------------------------------------------------------------------
def test_a_frame_cut_in_two_at_every_position():
    """one frame behind 300 quiet bits, cut at each of the 145 positions from the sync word's first bit to the header's last"""
    rng = np.random.default_rng(2)
    fb = im.frame_bits(im.random_header(rng))
    bits = plant(noise(600, 21), 300, fb)
    want = im.run(bits, 0)[0]
    assert len(want) == 1 and want[0]["pos"] == 323
    rx = rr.Il2pReceiver(1)                       # one handle for all cuts: 600 bits on, the stream rule has forgotten the frame before
    for k, cut in enumerate(range(300, 445)):
        got = run_device(rx, [bits], [(cut, [cut]), (600 - cut, [600 - cut])])
        rec = ic.record(want[0], 0)
        rec = (0, rec[1] + 600 * k) + rec[2:]
        assert got == ([[], [rec]] if cut < 444 else [[rec], []]), cut          # (cut 444: behind the header's last bit)
    assert rx.stats().tolist() == [[145, 145]]
    for cut in (300, 323, 324, 443, 444):         # and from a fresh handle against the model
        check([bits], [(cut, [cut]), (600 - cut, [600 - cut])])


# ---- 3. the chain rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner,accepted", [(120, False), (121, True)])
def test_a_sync_word_inside_a_header(inner, accepted):
    """a complete sync word planted so that its tag stands at p + 120 (the header's last bit: dropped) or p + 121 (the first free
    position: accepted, and its header decoded)"""
    rng = np.random.default_rng(3)
    bits = plant(noise(700, 31), 100, im.frame_bits(im.random_header(rng)))
    p = 123
    plant(bits, p + inner - 23, im.SYNC_WORD)
    want, stats = check([bits], [(700, [700])])
    assert [r[1] for r in want[0]] == ([p, p + 121] if accepted else [p]) and stats == [(2 if accepted else 1, 2)]
    check([bits], ic.even_pushes([bits], 97))


def test_back_to_back_frames_and_a_header_one_bit_short():
    rng = np.random.default_rng(4)
    fbs = [im.frame_bits(im.random_header(rng)) for _ in range(4)]
    bits = np.concatenate([noise(50, 41)] + [np.array(f, np.uint8) for f in fbs]).astype(np.uint8)       # gap 0
    want, stats = check([bits], [(len(bits), [len(bits)])])
    assert [r[1] for r in want[0]] == [73 + 144 * k for k in range(4)] and stats == [(4, 4)]
    check([bits], ic.even_pushes([bits], 144))
    # the stream ends 1 bit short of the last header, then gets that bit; and a stream that never gets it
    n = len(bits)
    want, stats = check([bits], [(n - 1, [n - 1]), (1, [1])])
    assert len(want[0]) == 3 and len(want[1]) == 1 and stats == [(4, 4)]
    want, stats = check([bits[:n - 1]], [(n - 1, [n - 1])])
    assert len(want[0]) == 3 and stats == [(3, 4)]


# ---- 4. tile seams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["sync word", "header"])
@pytest.mark.parametrize("first", [0, 1, 63, 64])
def test_tile_seams(first, what):
    """a sync word with its last bit at tile_bits - 24 .. tile_bits + 24 and a header starting at tile_bits - 121 .. tile_bits + 1,
    in a push of 2 tile_bits + 77 symbols, behind a first push of 0, 1, 63 and 64 symbols; one stream per placement"""
    T, carry = rr.Il2pReceiver(1).dims()
    assert T % 64 == 0 and carry >= 143
    n = 2 * T + 77
    rng = np.random.default_rng(5)
    hdr = im.random_header(rng)
    # (the tag stands one bit before the header)
    last_bits = list(range(T - 24, T + 25)) if what == "sync word" else [s - 1 for s in range(T - 121, T + 2)]
    quiet = noise(first + n, 500)
    streams = []
    for last in last_bits:
        b = quiet.copy()
        plant(b, first + last - 23, im.frame_bits(hdr))
        plant(b, first + T + 900, im.frame_bits(hdr))      # and a frame wholly inside the second tile
        streams.append(b)
    pushes = ([(first, [first] * len(streams))] if first else []) + [(n, [n] * len(streams))]
    want, stats = check(streams, pushes)
    assert stats == [(2, 2)] * len(streams)


# ---- 5. allowed_diffs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("allowed", [0, 1, 3])
def test_allowed_diffs_and_the_recorded_diffs(allowed):
    rng = np.random.default_rng(6)
    bits = noise(5 * 400, 61, allowed)
    for nflip in range(5):
        flips = rng.choice(24, nflip, replace=False).tolist()
        plant(bits, 400 * nflip + 50, im.frame_bits(im.random_header(rng), flips))
    want, stats = check([bits], [(len(bits), [len(bits)])], allowed=allowed)
    accepted = [(r[1], r[2]) for r in want[0]]
    assert [a for a in accepted if (a[0] - 73) % 400 == 0] == [(400 * k + 73, k) for k in range(min(allowed, 4) + 1)]
    check([bits], ic.even_pushes([bits], 333), allowed=allowed)


@pytest.mark.parametrize("allowed", [24, 1000])
def test_every_position_matches(allowed):
    """allowed_diffs 24 and above on random bits: the dense worst case and the start-of-stream rule in one: tags at every position
    from 23 on, headers at 23, 144, 265, ..."""
    n = 9000
    bits = np.random.default_rng(7).integers(0, 2, n).astype(np.uint8)
    want, stats = check([bits], [(n, [n])], allowed=allowed)
    assert [r[1] for r in want[0]] == list(range(23, n - 120, 121)) and stats == [(len(want[0]), n - 23)]
    check([bits], [(10, [10]), (13, [13]), (1, [1]), (n - 24, [n - 24])], allowed=allowed)


# ---- 6. the slicer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
def test_slicer_specials(invert):
    """NaN, +Inf, -Inf, +0.0, -0.0 and denormals in the sync word and in the header: only x > 0.0 is a 1 (before the inversion)"""
    rng = np.random.default_rng(8)
    bits = plant(noise(400, 81), 100, im.frame_bits(im.random_header(rng)))
    x = im.symbols(bits, invert)
    ones, zeros = [np.inf, 1e-45, 1e-39, 3e38], [np.nan, -np.inf, 0.0, -0.0, -1e-45, -1e-39]
    for i in range(90, 260):
        pool = ones if x[i] > 0 else zeros
        x[i] = pool[i % len(pool)]
    rx = rr.Il2pReceiver(1, invert=invert)
    got = ic.device_records(rx.push(x))
    want = [ic.record(h, 0) for h in im.run(bits, 0)[0]]
    assert got == want and len(want) == 1
    # the specials stand for the bits the model ran on
    with np.errstate(invalid="ignore"):
        assert np.array_equal((x > 0).astype(np.uint8) ^ (1 if invert else 0), bits)


# ---- 7. N streams ---------------------------------------------------------------------------------------------------------------------
def _ragged_streams(ns, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(ns):
        b = rng.integers(0, 2, n).astype(np.uint8)
        for at in range(int(rng.integers(0, 200)), n - 144, 300 + 7 * (c % 11)):
            plant(b, at, im.frame_bits(im.random_header(rng)))
        out.append(b)
    return out


@pytest.mark.parametrize("ns", [3, 65])
def test_streams_with_ragged_counts_on_the_device(ns):
    """counts 0, 1, n_cap and above n_cap (clamped) read on the device; every stream equals the single-stream handle on its own bits;
    a stream with count 0 keeps its open header across pushes; then the counts == NULL form"""
    n_cap, stride = 1000, 1003
    streams = _ragged_streams(ns, 5 * n_cap, 70 + ns)
    # stream 0 is cut inside a header by the first push and then pauses for two pushes
    streams[0][560:1100] = np.arange(540) & 1
    plant(streams[0], n_cap - 200, im.frame_bits(im.build_header()))
    plant(streams[0], n_cap - 60, im.frame_bits(im.random_header(np.random.default_rng(9))))
    rng = np.random.default_rng(71)
    table = [[n_cap] * ns]
    for k in range(3):
        row = [int(rng.choice([0, 1, n_cap, n_cap + 5, 1 << 40, int(rng.integers(0, n_cap))])) for _ in range(ns)]
        row[0] = 0 if k < 2 else n_cap
        table.append(row)
    rx = rr.Il2pReceiver(ns)
    singles = [rr.Il2pReceiver(1) for _ in range(min(ns, 5))]
    at = [0] * ns
    pushes, gots = [], []
    for row in table:
        took = [min(k, n_cap) for k in row]
        a = np.full((ns, stride), np.nan, np.float32)                     # NaN behind the counts: never read
        for c in range(ns):
            a[c, :took[c]] = im.symbols(streams[c][at[c]:at[c] + took[c]])
        d_syms = torch.from_numpy(a).cuda()
        d_counts = torch.from_numpy(np.array(row, np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()
        rx.push_dev(d_syms.data_ptr(), stride, n_cap, d_counts.data_ptr())
        got = ic.device_records(rx.headers())
        for c, one in enumerate(singles):
            mine = ic.device_records(one.push(a[c, :took[c]])) if took[c] else []
            assert [r[1:] for r in got if r[0] == c] == [r[1:] for r in mine], c
        pushes.append((n_cap, took))
        gots.append(got)
        at = [x + t for x, t in zip(at, took)]
    want = ic.expected(streams, pushes, 0)
    assert gots == want[0]
    assert rx.consumed().tolist() == at
    assert [tuple(int(v) for v in r) for r in rx.stats()] == want[1]
    # stream 0's second frame began in push 0 and ended in push 3, two pauses later
    assert any(r[0] == 0 and r[1] == n_cap - 60 + 23 for r in want[0][3]) and not any(r[0] == 0 for r in want[0][1] + want[0][2])
    # counts == NULL: every stream has n_cap
    rest = [s[at[c]:at[c] + 500] for c, s in enumerate(streams)]
    assert all(len(r) == 500 for r in rest)
    d = torch.from_numpy(np.stack([im.symbols(r) for r in rest])).cuda()
    torch.cuda.synchronize()
    rx.push_dev(d.data_ptr(), 500, 500, None)
    pushes.append((500, [500] * ns))
    want = ic.expected(streams, pushes, 0)
    assert ic.device_records(rx.headers()) == want[0][-1] and len(want[0][-1]) > 0
    # a push of nothing: no launch, no headers, every state kept
    rx.push_dev(0, 0, 0, None)
    assert len(rx.headers()) == 0 and rx.consumed().tolist() == [sum(p[1][c] for p in pushes) for c in range(ns)]


def test_symbol_sync_counts_fed_straight_to_push_dev():
    """rr_symbol_sync_push_dev's symbols and rr_symbol_sync_counts_dev's counts go to push_dev without a host in between; the
    model runs on the symbols downloaded afterwards"""
    ns, sps = 3, 4
    rng = np.random.default_rng(10)
    rows = []
    for c in range(ns):
        b = np.concatenate([np.arange(200 + 16 * c) & 1, im.frame_bits(im.random_header(rng)), np.arange(64) & 1,
                            im.frame_bits(im.random_header(rng)), np.arange(60) & 1]).astype(np.uint8)
        rows.append(np.repeat(im.symbols(b), sps))
    n = max(len(r) for r in rows)
    x = np.stack([np.concatenate([r, np.full(n - len(r), r[-1], np.float32)]) for r in rows])
    ss = rr.SymbolSync(float(sps), 0.0, [0.0001, 0.99999999], nstreams=ns)
    rx = rr.Il2pReceiver(ns)
    d_in = torch.from_numpy(x).cuda()
    d_syms = torch.zeros((ns, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ss.push_dev(d_in.data_ptr(), n, n, d_syms.data_ptr(), None, n, s)
    rx.push_dev(d_syms.data_ptr(), n, n, ss.counts_dev(), s)
    got = ic.device_records(rx.headers())
    counts = ss.produced()
    syms = d_syms.cpu().numpy()
    want = []
    for c in range(ns):
        hs, _ = im.run((syms[c, :int(counts[c])] > 0).astype(np.uint8), 0)
        assert len(hs) == 2, c
        want += [ic.record(h, c) for h in hs]
    assert got == want and rx.consumed().tolist() == [int(k) for k in counts]


# ---- 8. the launch count --------------------------------------------------------------------------------------------------------------
def test_launch_count():
    """the same number of launches for 1 and 4,096 streams, for silence, one frame and allowed_diffs 24; none for n_cap == 0"""
    L = rr.lib()
    n = 300
    frame = plant(np.zeros(n, np.uint8), 40, im.frame_bits(im.build_header()))
    seen = set()
    for ns in (1, 4096):
        for allowed, bits in ((0, np.zeros(n, np.uint8)), (0, frame), (24, frame)):
            rx = rr.Il2pReceiver(ns, allowed_diffs=allowed)
            a = np.tile(im.symbols(bits), (ns, 1))
            rx.push(a)                                                    # (the first push allocates)
            before = L.rr_debug_kernel_launches()
            rec = rx.push(a)
            seen.add(L.rr_debug_kernel_launches() - before)
            assert len(rec) == ns * len(im.run(np.concatenate([bits, bits]), allowed)[0]) - ns * len(im.run(bits, allowed)[0])
            before = L.rr_debug_kernel_launches()
            assert len(rx.push(np.zeros((ns, 0), np.float32))) == 0
            assert L.rr_debug_kernel_launches() == before
    assert len(seen) == 1 and 0 < seen.pop() <= 4


# ---- 9. seeded fuzz -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ic.FUZZ_SEEDS)
def test_seeded_fuzz(seed):
    streams, pushes, allowed, invert = ic.fuzz_case(seed)
    check(streams, pushes, allowed=allowed, invert=invert)


# ---- 10. through the transmitter ------------------------------------------------------------------------------------------------------
def test_loopback_through_the_transmitter():
    """rr_fsk_tx (bell202: 1200 / 2200 Hz at 12 kS/s) -> rr_afsk_demod -> rr_symbol_sync -> rr_il2p_receiver_push_dev on one HIP
    stream, the counts staying on the device.  Polarity: rr_fsk_tx sends a 1 as the HIGHER tone and the demodulator's offset of
    -1700 Hz leaves that positive, so the receiver runs WITHOUT inversion (il2p-1200-rx.rs inverts because Bell 202's mark, its 1,
    is the lower tone).  Both headers come back with their raw bytes as sent."""
    line, sent = ic.loopback_line()
    t = fk.LOOP_TX
    tx = rr.FskTx(rr.FSK_TX_AFSK, t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])
    na, no = tx.count(len(line))
    d_bits = torch.from_numpy(line).cuda()
    audio = torch.zeros(na, dtype=torch.float32, device="cuda")
    out = torch.zeros(max(no, 1), dtype=torch.complex64, device="cuda")
    soft = torch.zeros(na, dtype=torch.float32, device="cuda")
    syms = torch.zeros(na, dtype=torch.float32, device="cuda")
    af = rr.AfskDemod(1, am.HIL, am.taps12k(), am.GAIN, am.OFFSET)
    ss = rr.SymbolSync(*am.SYNC_PRM, nstreams=1)
    rx = rr.Il2pReceiver(1, invert=False)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    tx.push_dev(d_bits.data_ptr(), len(line), out.data_ptr(), no, audio.data_ptr(), na, s)
    p = af.push_dev(audio.data_ptr(), na, na, soft.data_ptr(), na, s)
    ss.push_dev(soft.data_ptr(), na, p, syms.data_ptr(), None, na, s)
    rx.push_dev(syms.data_ptr(), na, p, ss.counts_dev(), s)
    rec = rx.headers()                                                    # (waits for all four)
    assert [r["raw"].tobytes() for r in rec] == sent
    assert rec[0]["dst"] == b"2E0QQQ" and rec[0]["src"] == b"M0THC" and int(rec[1]["pos"]) - int(rec[0]["pos"]) == 144
    assert rx.stats().tolist() == [[2, 2]]
