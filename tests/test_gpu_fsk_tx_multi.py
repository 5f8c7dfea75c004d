"""GPU: rr.FskTxMulti (rr_fsk_tx_multi_*, kernels_tx.hip) against rr.FskTx itself (bit for bit wherever both take the
general path), the bounds of tests/fsk_model.py where they do not, and the library's own receivers: independence of a stream from
everything that is not its own bits, nothing written beyond a stream's counts, launch counts, the second chunk of the tile-level
scans, framer -> modulator with no host read, and three stations through AfskDemod(3) -> SymbolSync(3) -> HdlcReceiver(3)."""
import math

import numpy as np
import pytest
import torch

import afsk_model as am
import fsk_dev as fd
import fsk_model as fk
import fsk_multi_dev as fmd
import rustradio_amd as rr

pytestmark = pytest.mark.gpu

K1, K2 = 2.0 * math.pi / 12000.0, 2.0 * math.pi * 5000.0 / 48000.0
TX = (1200.0, 2200.0, K1, 0.5, K2)             # lo, hi, k1, gain, k2
MODES = [rr.FSK_TX_AFSK, rr.FSK_TX_DIRECT]
MODE_IDS = ["afsk", "direct"]
LD = np.longdouble


def multi(n, mode, sh, tx=TX):
    lo, hi, k1, gain, k2 = tx
    return rr.FskTxMulti(n, mode, sh[0], sh[1], lo, hi, k1, gain, sh[2], sh[3], k2)


def single(mode, sh, tx=TX):
    lo, hi, k1, gain, k2 = tx
    return rr.FskTx(mode, sh[0], sh[1], lo, hi, k1, gain, sh[2], sh[3], k2)


def dims():
    return multi(1, rr.FSK_TX_AFSK, (10, 1, 4, 1)).dims()


def stream0():
    return torch.cuda.current_stream().cuda_stream


def need(r1, pos, target):
    """the fewest bits behind `pos` that make at least `target` audio samples"""
    n = 1
    while fk.made(pos + n, *r1) - fk.made(pos, *r1) < target:
        n += 1
    return n


def most(r1, pos, target):
    """the most bits behind `pos` that make at most `target` audio samples (at least one bit)"""
    n = 1
    while fk.made(pos + n + 1, *r1) - fk.made(pos, *r1) <= target:
        n += 1
    return n


def test_dims_and_bound():
    assert dims() == (2048, 2048, 4096)
    h = multi(3, rr.FSK_TX_AFSK, (40, 1, 25, 24))
    assert h.bound(0) == (0, 0) and h.bound(7) == (280, 292) and h.bound(1) == (40, 42)
    assert multi(2, rr.FSK_TX_DIRECT, (3, 7, 3, 7)).bound(5) == (3, 2)


# ---- 1. the same bits as the one-stream handle -----------------------------------------------------------------------------------------
KINDS = [["zero", "several", "zero"], ["mod1", "onebit", "tile1"], ["tile1", "several", "cap"], ["cap", "zero", "several"],
         ["several", "over", "tile1"]]


def schedule(sh, atile):
    """-> (n_cap, [[(count given, bits taken) per push] per stream]): every push of every stream makes no audio sample or more than
    one audio tile, so rr.FskTx takes its general path too"""
    r1 = fk.reduced(sh[0], sh[1])
    n_cap = need(r1, 0, 3 * atile + 17) + 64
    plan = []
    for kinds in KINDS:
        pos, mine = 0, []
        for kind in kinds:
            if kind == "zero":
                k = 0
            elif kind == "onebit":             # a bit that makes no audio sample, where the ratio has one
                k = 1 if r1[1] > 1 else 0
            elif kind == "tile1":
                k = need(r1, pos, atile + 1)
            elif kind == "mod1":               # ... and leaves the stream where its next bit makes none (3:7: positions 1 mod 7)
                k = need(r1, pos, atile + 1)
                while r1[1] > 1 and (pos + k) % r1[1] != 1:
                    k += 1
            elif kind == "several":
                k = need(r1, pos, 2 * atile + 5)
            else:
                k = n_cap + (1000 if kind == "over" else 0)
            n = min(k, n_cap)
            na = fk.made(pos + n, *r1) - fk.made(pos, *r1)
            assert na == 0 or na > atile, (kind, na)
            if kind == "onebit" and k:
                assert na == 0
            if kind == "tile1" and r1 == (3, 7):
                assert na == atile + 1
            mine.append((k, n))
            pos += n
        plan.append(mine)
    return n_cap, plan


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("sh", [(10, 1, 4, 1), (3, 7, 3, 7)], ids=["10:1-4:1", "3:7-3:7"])
def test_same_bits_as_the_one_stream_handle(sh, mode):
    """N = 5, three pushes; counts 0, one bit that makes no audio (3:7), audio_tile + 1 samples (the fewest above a tile where the
    ratio has no such count), several tiles, exactly n_cap and a count above it: out, audio and counts bit-identical to five
    rr.FskTx handles given the same pushes; positions() is fk.counts"""
    atile, _, _ = dims()
    afsk = mode == rr.FSK_TX_AFSK
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    n_cap, plan = schedule(sh, atile)
    N = len(plan)
    bits = [fk.patterns(sum(n for _, n in plan[c]), 300 + c)["random"] for c in range(N)]
    h, ones, at = multi(N, mode, sh), [single(mode, sh) for _ in range(N)], [0] * N
    for p in range(3):
        rows = [bits[c][at[c]:at[c] + plan[c][p][1]] for c in range(N)]
        outs, auds, made, nl = fmd.multi_push(h, rows, [plan[c][p][0] for c in range(N)], n_cap=n_cap, audio=afsk)
        assert nl == (6 if afsk else 5)
        for c in range(N):
            o1, a1, _ = fd.dev_push(ones[c], rows[c], audio=afsk)
            assert fd.same_bits(outs[c], o1.cpu().numpy()), (p, c)
            if afsk:
                assert fd.same_bits(auds[c], a1.cpu().numpy()), (p, c)
            want = fk.counts([n for _, n in plan[c][:p + 1]], r1, r2)[-1]
            assert (int(made[c, 0]), int(made[c, 1])) == want, (p, c)
            at[c] += plan[c][p][1]
    pos = h.positions()
    for c in range(N):
        cnt = fk.counts([n for _, n in plan[c]], r1, r2)
        assert tuple(int(v) for v in pos[c]) == (at[c], sum(a for a, _ in cnt), sum(o for _, o in cnt)), c


# ---- 2. bounds where the two handles take different paths -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("sh", [(10, 1, 4, 1), (3, 7, 3, 7)], ids=["10:1-4:1", "3:7-3:7"])
def test_short_pushes_meet_the_bounds(sh, mode):
    """streams whose pushes make 1 .. audio_tile samples: rr.FskTx runs its one-tile kernels there, this handle the general path,
    so they are judged by the three bounds (AFSK outputs against the truth from the a[] the same pushes wrote), from the stream's
    start over two pushes"""
    atile, _, _ = dims()
    afsk = mode == rr.FSK_TX_AFSK
    lo, hi, k1, gain, k2 = TX
    r1, r2 = fk.reduced(sh[0], sh[1]), fk.reduced(sh[2], sh[3])
    targets = [[1, atile], [7, atile - 3], [atile - 1, 5], [atile, 1], [atile // 2, atile // 3]]
    N = len(targets)
    lens = []
    for t in targets:
        n0 = most(r1, 0, t[0])
        lens.append([n0, most(r1, n0, t[1])])
    for c in range(N):
        for a, _ in fk.counts(lens[c], r1, r2):
            assert 1 <= a <= atile
    bits = [fk.patterns(sum(lens[c]), 400 + c)["random"] for c in range(N)]
    h, at = multi(N, mode, sh), [0] * N
    outs, auds = [[] for _ in range(N)], [[] for _ in range(N)]
    for p in range(2):
        rows = [bits[c][at[c]:at[c] + lens[c][p]] for c in range(N)]
        o, a, made, _ = fmd.multi_push(h, rows, [lens[c][p] for c in range(N)], audio=afsk)
        for c in range(N):
            assert (int(made[c, 0]), int(made[c, 1])) == fk.counts(lens[c][:p + 1], r1, r2)[-1]
            outs[c].append(o[c])
            if afsk:
                auds[c].append(a[c])
            at[c] += lens[c][p]
    for c in range(N):
        out = np.concatenate(outs[c])
        if afsk:
            aud = np.concatenate(auds[c])
            ua, ta = fk.used_audio(aud, bits[c], r1, lo, hi, k1, gain)
            uo, to = fk.used_out(out, aud, r2, k2)
        else:
            ua, ta = fk.used_direct(out, fk.made(len(bits[c]), *r1), bits[c], r1, r2, lo, hi, k1, gain)
            uo, to = 0.0, 0.0
        print(f"stream {c}: used {ua:.4f} (stage 1 / DIRECT) {uo:.4f} (AFSK out); truths' own {ta:.1e} {to:.1e}")
        assert ta <= 0.01 and to <= 0.01, c
        assert ua <= 1.0 and uo <= 1.0, c


# ---- 3. independence -------------------------------------------------------------------------------------------------------------------
def _two_pushes(mode, sh, rows_of, N=1, at=0, **kw):
    """two pushes of the stream under test (index `at` of N) -> (out, audio) of that stream, each the two pushes' back to back;
    rows_of(p) -> (rows, counts, n_cap) of push p"""
    h, outs, auds = multi(N, mode, sh), [], []
    afsk = mode == rr.FSK_TX_AFSK and kw.get("audio", True)
    for p in range(2):
        rows, counts, n_cap = rows_of(p)
        o, a, _, _ = fmd.multi_push(h, rows, counts, n_cap=n_cap, **{"audio": afsk, **{k: v for k, v in kw.items() if k != "audio"}})
        outs.append(o[at])
        if afsk:
            auds.append(a[at])
    return np.concatenate(outs), (np.concatenate(auds) if afsk else None)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_stream_depends_on_nothing_but_its_own_bits(mode):
    """one stream's bits are the same for N = 1 and N = 7 with the other streams' bits and counts random, for larger strides, for an
    n_cap of twice the need, with d_counts NULL or equal to n_cap, with and without d_audio; a count above n_cap is clamped; an
    all-zero-count push between the two changes nothing a later push can see"""
    sh = (10, 1, 4, 1)
    afsk = mode == rr.FSK_TX_AFSK
    lens = [330, 41]                           # more than one audio tile, then fewer
    mine = fk.patterns(sum(lens), 501)["random"]
    part = [mine[:lens[0]], mine[lens[0]:]]
    base_o, base_a = _two_pushes(mode, sh, lambda p: ([part[p]], [lens[p]], lens[p]))
    same = lambda o, a: fd.same_bits(o, base_o) and (not afsk or a is None or fd.same_bits(a, base_a))
    rng = np.random.default_rng(7)

    def among_seven(p):
        rows = [rng.integers(0, 2, lens[p], dtype=np.uint8) for _ in range(7)]
        counts = [int(v) for v in rng.integers(0, lens[p] + 1, 7)]
        rows[3], counts[3] = part[p], lens[p]
        return rows, counts, lens[p]
    assert same(*_two_pushes(mode, sh, among_seven, N=7, at=3)), "N = 7"
    ac, oc = multi(1, mode, sh).bound(max(lens))
    assert same(*_two_pushes(mode, sh, lambda p: ([part[p]], [lens[p]], lens[p]), bits_stride=max(lens) + 13, out_stride=oc + 1000,
                             audio_stride=ac + 77)), "strides"
    assert same(*_two_pushes(mode, sh, lambda p: ([part[p]], [lens[p]], 2 * lens[p]))), "n_cap twice the need"
    assert same(*_two_pushes(mode, sh, lambda p: ([part[p]], [lens[p]], lens[p]), null_counts=True)), "d_counts NULL"
    assert same(*_two_pushes(mode, sh, lambda p: ([part[p]], [lens[p] + 5], lens[p]))), "a count above n_cap"
    if afsk:
        assert same(*_two_pushes(mode, sh, lambda p: ([part[p]], [lens[p]], lens[p]), audio=False)), "d_audio NULL"
    # an all-zero-count push in between
    h = multi(2, mode, sh)
    o1, a1, _, _ = fmd.multi_push(h, [part[0], part[0][:5]], [lens[0], 5], audio=afsk)
    before = h.positions()
    oz, _, made, nl = fmd.multi_push(h, [mine[:50], mine[:50]], [0, 0], audio=afsk)
    assert nl == (6 if afsk else 5) and not made.any() and all(len(v) == 0 for v in oz)
    assert np.array_equal(h.positions(), before)
    o2, a2, _, _ = fmd.multi_push(h, [part[1], part[1][:3]], [lens[1], 3], audio=afsk)
    assert same(np.concatenate([o1[0], o2[0]]), np.concatenate([a1[0], a2[0]]) if afsk else None), "zero-count push"


# ---- 4. nothing beyond the counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_nothing_is_written_at_or_beyond_a_streams_own_counts(mode):
    """ragged counts under wide strides: fsk_multi_dev.multi_push finds the sentinel in every element from each stream's own n_out /
    n_audio up to its stride; a stream of count 0 owns a row of sentinels"""
    atile, _, _ = dims()
    sh = (40, 1, 25, 24)
    counts = [0, 1, 52, 3, 160, 17]            # 40 .. 6400 audio samples: below, at and above one tile
    n_cap = 160
    rows = [fk.patterns(n_cap, 600 + c)["random"] for c in range(len(counts))]
    h = multi(len(counts), mode, sh)
    ac, oc = h.bound(n_cap)
    for _ in range(2):
        outs, auds, made, _ = fmd.multi_push(h, rows, counts, n_cap=n_cap, audio=mode == rr.FSK_TX_AFSK, out_stride=oc + 4 * atile + 3,
                                             audio_stride=ac + atile + 5)
        assert [int(v) for v in made[:, 0]] == [40 * k for k in counts]
        assert len(outs[0]) == 0 and all(len(o) == int(m) for o, m in zip(outs, made[:, 1]))


# ---- 5. launches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_launches_depend_on_the_mode_alone(mode):
    atile, _, _ = dims()
    afsk = mode == rr.FSK_TX_AFSK
    sh, n_cap = (10, 1, 4, 1), 260             # one stream's push: more than one audio tile
    seen = set()
    for N in (1, 64):
        for name in ("zeros", "ones", "alt", "random"):
            rows = [fk.patterns(n_cap, 700 + c)[name] for c in range(N)]
            h = multi(N, mode, sh)
            for counts in ([0] * N, [n_cap] * N, [int(v) for v in np.random.default_rng(N).integers(0, n_cap + 1, N)]):
                seen.add(fmd.multi_push(h, rows, counts, n_cap=n_cap, audio=afsk)[3])
    assert len(seen) == 1 and seen.pop() <= (6 if afsk else 5)
    h = multi(3, mode, sh)
    torch.cuda.synchronize()
    l0 = fd.launches()
    h.push_dev(0, 0, 0, None, 0, 0)            # n_cap == 0 needs no buffers and launches nothing
    assert fd.launches() == l0
    assert not h.counts().any() and not h.positions().any()


# ---- 6. the second chunk of the tile-level scans ------------------------------------------------------------------------------------------------
def test_second_scan_chunk():
    """N = 2, 1:1 / 1:1 AFSK: one stream has more audio tiles than one pass of the tile-level scans takes, the other 100 bits.  The
    long stream equals rr.FskTx bit for bit; 16 segments of it, both sides of the chunk seam among them, and the short stream meet
    the bounds (stage 1 against the counts' exact phase, stage 2 against the long-double sum over the push's own audio)"""
    atile, _, chunk = dims()
    sh, n = (1, 1, 1, 1), atile * chunk + 5000
    tx = (-1.0, 2.0, 0.37, 0.5, 0.61)
    lo, hi, k1, gain, k2 = tx
    bits, short = fk.patterns(n, 77)["random"], fk.patterns(100, 78)["random"]
    outs, auds, made, nl = fmd.multi_push(multi(2, rr.FSK_TX_AFSK, sh, tx), [bits, short], [n, 100], n_cap=n)
    assert nl == 6 and made.tolist() == [[n, n], [100, 100]]
    o1, a1, _ = fd.dev_push(single(rr.FSK_TX_AFSK, sh, tx), bits)
    assert fd.same_bits(outs[0], o1.cpu().numpy()) and fd.same_bits(auds[0], a1.cpu().numpy())
    del o1, a1
    seam, seg = atile * chunk, 256
    starts = [0, seam - seg, seam, n - seg] + [int(v) for v in np.linspace(atile + 11, n - 2 * seg, 12)]
    sel = np.unique(np.concatenate([np.arange(s, s + seg) for s in starts])).astype(np.int64)
    assert len(starts) == 16 and seam - 1 in sel and seam in sel
    uo, to = fk.used_out(outs[0][sel], auds[0], (1, 1), k2, sel)
    c1 = np.cumsum(bits != 0, dtype=np.int64)[sel]
    ph = LD(float(k1)) * (LD(np.float32(hi)) * c1.astype(LD) + LD(np.float32(lo)) * (sel + 1 - c1).astype(LD))
    sn, _ = fk._sincos(ph)
    d1 = fk.d1_of(lo, hi, k1)
    b = fk.audio_bound(sel, gain, d1)
    ua = float(np.max(np.abs(auds[0][sel].astype(LD) - LD(np.float32(gain)) * sn).astype(np.float64) / b))
    ta = abs(gain) * fk.truth1_error(n, d1) / float(b[0])
    print(f"long stream, 16 segments: used {ua:.4f} (stage 1) {uo:.4f} (out); truths' own {ta:.1e} {to:.1e}")
    assert ta <= 0.01 and to <= 0.01 and ua <= 1.0 and uo <= 1.0
    ua, ta = fk.used_audio(auds[1], short, (1, 1), lo, hi, k1, gain)
    uo, to = fk.used_out(outs[1], auds[1], (1, 1), k2)
    print(f"short stream: used {ua:.4f} (stage 1) {uo:.4f} (out)")
    assert ta <= 0.01 and to <= 0.01 and ua <= 1.0 and uo <= 1.0


# ---- 7, 8. framer -> modulator with no host read, and into the library's own receivers --------------------------------------------------------
class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def frame_on_device(packet_sets, n_cap, d_bits, s):
    """one HdlcFramer(FCS | NRZI) per packet set, its bits to row p of d_bits (n_cap wide) -> the framers (kept alive: their
    produced words are read later on the stream)"""
    framers = []
    for p, packets in enumerate(packet_sets):
        fr = rr.HdlcFramer(fk.LOOP_FLAGS)
        lens = np.array([len(q) for q in packets], np.uintp)
        starts = (np.cumsum(lens) - lens).astype(np.uintp)
        assert fr.bound(lens) == fmd.framer_bound(packets) <= n_cap
        d_bytes = torch.from_numpy(np.frombuffer(b"".join(packets), np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        fr.push_dev(d_bytes.data_ptr(), int(lens.sum()), starts, lens, d_bits[p].data_ptr(), n_cap, s)
        framers.append((fr, d_bytes))
    return framers


def receive(d_audio, N, n):
    """AfskDemod(N) -> SymbolSync(N) -> HdlcReceiver(N, nrzi) over n device samples of each row -> ([[payload] per stream], stats)"""
    af = rr.AfskDemod(N, am.HIL, am.taps12k(), am.GAIN, am.OFFSET)
    ss = rr.SymbolSync(*am.SYNC_PRM, nstreams=N)
    rx = rr.HdlcReceiver(N, 1, am.MAX_SIZE, nrzi=True)
    soft = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    syms = torch.zeros((N, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = stream0()
    p = af.push_dev(d_audio.data_ptr(), n, n, soft.data_ptr(), n, s)
    ss.push_dev(soft.data_ptr(), n, p, syms.data_ptr(), None, n, s)
    rx.push_dev(syms.data_ptr(), n, p, ss.counts_dev(), s)
    frames = [[f[1] for f in per] for per in rx.result()]            # (waits for all three)
    return frames, [tuple(int(v) for v in row) for row in rx.stats()]


def transmit(packet_sets):
    """framers -> FskTxMulti(len(packet_sets)) on one stream with no host read in between -> (audio tensor (N, audio_cap), zeroed
    behind every stream's own count; the handle; audio_cap)"""
    N = len(packet_sets)
    t = fk.LOOP_TX
    n_cap = max(fmd.framer_bound(ps) for ps in packet_sets)
    tx = rr.FskTxMulti(N, rr.FSK_TX_AFSK, t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])
    ac, oc = tx.bound(n_cap)
    assert (ac, oc) == (10 * n_cap, 40 * n_cap)
    d_bits = torch.zeros((N, n_cap), dtype=torch.uint8, device="cuda")
    audio = torch.zeros((N, ac), dtype=torch.float32, device="cuda")
    out = torch.zeros((N, oc), dtype=torch.complex64, device="cuda")
    d_counts = torch.zeros(8 * N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = stream0()
    framers = frame_on_device(packet_sets, n_cap, d_bits, s)
    if N == 1:
        counts_ptr = framers[0][0].produced_dev()                    # the framer's own word is the count
    else:
        for p, (fr, _) in enumerate(framers):                        # N words gathered by 8-byte device copies on the same stream
            d_counts[8 * p:8 * p + 8].copy_(torch.as_tensor(_DevMem(fr.produced_dev(), 8), device="cuda"), non_blocking=True)
        counts_ptr = d_counts.data_ptr()
    l0 = fd.launches()
    tx.push_dev(d_bits.data_ptr(), n_cap, n_cap, counts_ptr, out.data_ptr(), oc, audio.data_ptr(), ac, s)
    assert fd.launches() - l0 == 6
    return audio, tx, ac, d_bits, framers


def test_framer_to_modulator_with_no_host_read():
    """HdlcFramer(FCS | NRZI).push_dev -> produced_dev() -> FskTxMulti(1).push_dev with n_cap = the framer's bound: the counts are
    the one-stream handle's for the framed bits, and the audio loop of test_gpu_fsk_tx_loopback.py returns the packets"""
    audio, tx, ac, d_bits, framers = transmit([fk.loop_packets()])
    n_bits = len(fk.loop_bits())
    t = fk.LOOP_TX
    one = rr.FskTx(rr.FSK_TX_AFSK, t["i1"], t["d1"], t["lo"], t["hi"], t["k1"], t["gain"], t["i2"], t["d2"], t["k2"])
    assert tuple(int(v) for v in tx.counts()[0]) == one.count(n_bits) == (10 * n_bits, 40 * n_bits)
    assert framers[0][0].records()[1] == n_bits
    assert np.array_equal(d_bits[0, :n_bits].cpu().numpy(), fk.loop_bits())
    assert not audio[0, 10 * n_bits:].any()
    frames, stats = receive(audio, 1, ac)
    assert frames[0] == fk.loop_packets()
    assert stats[0] == (len(frames[0]), 0, 0)


def test_three_stations():
    """three framers, their counts gathered by device copies, FskTxMulti(3) with audio into a zeroed buffer -> AfskDemod(3) ->
    SymbolSync(3) -> HdlcReceiver(3) on one stream: every station's packets come back once, in order, stats (n, 0, 0)"""
    sets = fmd.station_packets()
    audio, tx, ac, _, _ = transmit(sets)
    made = tx.counts()
    assert [int(v) for v in made[:, 0]] == [10 * len(b) for b in fmd.station_bits()]
    frames, stats = receive(audio, 3, ac)
    for c, packets in enumerate(sets):
        assert frames[c] == packets, c
        assert stats[c] == (len(packets), 0, 0), c


# ---- refusals and the host entry -----------------------------------------------------------------------------------------------------------
def test_push_refusals_launch_nothing_and_change_nothing():
    sh, n = (10, 1, 4, 1), 300
    bits = fk.patterns(2 * n, 31)["random"]
    h = multi(2, rr.FSK_TX_AFSK, sh)
    o1, a1, _, _ = fmd.multi_push(h, [bits[:n], bits[:n]], [n, n])
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, big = d.data_ptr(), 1 << 40
    l0 = fd.launches()
    P = "fsk tx multi: "
    # d_bits, bits_stride, n_cap, d_counts, d_out, out_stride, d_audio, audio_stride
    for args, msg in [((0, n, n, None, p, big, 0, 0), "null bit buffer"), ((p, n, n, None, 0, big, 0, 0), "null output buffer"),
                      ((p, n - 1, n, None, p, big, 0, 0), "bits_stride below n_cap"),
                      ((p, n, n, None, p, 40 * n - 1, 0, 0), "out_stride below the outputs a stream can make"),
                      ((p, n, n, None, p, big, p, 10 * n - 1), "audio_stride below the audio samples a stream can make"),
                      ((p, big, (1 << 30) + 1, None, p, big, 0, 0), "more than 2\\^30 bits of a stream in one push"),
                      ((p, big, (1 << 30) // 20 + 1, None, p, big, 0, 0), "more than 2\\^30 audio samples of all streams in one push"),
                      ((p, big, (1 << 30) // 80 + 1, None, p, big, 0, 0), "more than 2\\^30 outputs of all streams in one push")]:
        with pytest.raises(ValueError, match=P + msg):
            h.push_dev(*args)
    with pytest.raises(ValueError, match=P + "DIRECT mode has no audio output"):
        multi(2, rr.FSK_TX_DIRECT, sh).push_dev(p, n, n, None, p, big, p, big)
    assert fd.launches() == l0
    o2, a2, _, _ = fmd.multi_push(h, [bits[n:], bits[n:]], [n, n])
    w = single(rr.FSK_TX_AFSK, sh)
    wo, wa, _ = fd.run_pushes(w, bits, [n, n])
    for c in range(2):
        assert fd.same_bits(np.concatenate([o1[c], o2[c]]), wo) and fd.same_bits(np.concatenate([a1[c], a2[c]]), wa)
    with pytest.raises(RuntimeError, match="FskTxMulti takes pushes of line bits"):     # rr_block_work on the handle is an error
        h.work(np.zeros(4, np.uint8), 16)


def test_host_push_equals_device_push():
    sh, n = (10, 1, 4, 1), 700
    rows = np.stack([fk.patterns(n, 41 + c)["random"] for c in range(3)])
    counts = [n, 0, 333]
    o, a = multi(3, rr.FSK_TX_AFSK, sh).push(rows, counts, audio=True)
    wo, wa, _, _ = fmd.multi_push(multi(3, rr.FSK_TX_AFSK, sh), list(rows), counts)
    for c in range(3):
        assert fd.same_bits(o[c], wo[c]) and fd.same_bits(a[c], wa[c])
    od = multi(3, rr.FSK_TX_DIRECT, sh).push(rows, counts)
    wd, _, _, _ = fmd.multi_push(multi(3, rr.FSK_TX_DIRECT, sh), list(rows), counts, audio=False)
    assert all(fd.same_bits(od[c], wd[c]) for c in range(3))
    assert [len(v) for v in multi(3, rr.FSK_TX_AFSK, sh).push(np.zeros((3, 0), np.uint8))] == [0, 0, 0]
