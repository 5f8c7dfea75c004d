"""GPU: rr_hdlc_receiver (kernels_hdlcrx.hip) — N symbol streams to checked frames — against the project's Python machines
(bits_model.Chain -> hdlc_model.HdlcModel) and the single-stream handles rr.BitDecoder -> rr.HdlcDeframer fed one stream at a time.
Every comparison is bit for bit: frames, bytes, positions, repaired flags, the three counters and the symbols consumed; there is no
tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import hdlc_model as hm
import hdlcrx_helpers as hx
import rustradio_amd as rr
from hdlc_model import FLAG, bytes_to_bits, frame_bits, stuff

pytestmark = pytest.mark.gpu
KEEP, FIX = rr.HDLC_KEEP_CHECKSUM, rr.HDLC_FIX_BITS


def launches():
    return rr.lib().rr_debug_kernel_launches()


def stream0():
    return torch.cuda.current_stream().cuda_stream


def make_rx(n, cfg):
    mn, mx, flags, line = cfg
    inv, nrzi, des = hx.LINE_CONFIGS[line]
    return rr.HdlcReceiver(n, mn, mx, invert=inv, nrzi=nrzi, descrambler=des, flags=flags)


class Single:
    """one stream through the single-stream handles"""

    def __init__(self, cfg):
        mn, mx, flags, line = cfg
        inv, nrzi, des = hx.LINE_CONFIGS[line]
        self.bd, self.df = rr.BitDecoder(invert=inv, nrzi=nrzi, descrambler=des), rr.HdlcDeframer(mn, mx, flags)
        self.taken = 0

    def push(self, syms):
        if len(syms) == 0:
            return []
        _, _, p, _, bits = self.bd.work(np.asarray(syms, np.float32), len(syms))
        assert p == len(syms)
        self.taken += p
        return self.df.push(bits)

    def stats(self):
        return tuple(self.df.stats())


def model(cfg):
    mn, mx, flags, line = cfg
    inv, nrzi, des = hx.LINE_CONFIGS[line]
    return hx.ModelReceiver(mn, mx, inv, nrzi, des, flags)


def snapshot(rx):
    return rx.result(), [tuple(int(v) for v in r) for r in rx.stats()], [int(v) for v in rx.consumed()]


def feed(rx, syms, counts=None, via="dev"):
    """one push of the rows of syms (f32[N, n_cap]) -> snapshot"""
    syms = np.ascontiguousarray(syms, np.float32)
    if via == "host":
        rx.push(syms, counts)
        return snapshot(rx)
    d = torch.from_numpy(syms).cuda()
    dc = torch.from_numpy(np.asarray(counts, np.uint64).view(np.int64)).cuda() if counts is not None else None
    rx.push_dev(d.data_ptr(), syms.shape[1], syms.shape[1], dc.data_ptr() if dc is not None else None, stream0())
    return snapshot(rx)                        # (waits: d and dc outlive the push)


def expect(oracles, syms, counts):
    """the same push through one oracle per stream -> snapshot"""
    n_cap = syms.shape[1]
    k = [n_cap] * len(oracles) if counts is None else [min(int(c), n_cap) for c in counts]
    frames = [o.push(syms[c, :k[c]]) for c, o in enumerate(oracles)]
    for c, o in enumerate(oracles):
        o.total = getattr(o, "total", 0) + k[c]
    return frames, [o.stats() for o in oracles], [o.total for o in oracles]


def plant(rng, lens, line, frame_bytes=30):
    """symbols of sum(lens) bits of a drawn stream with a frame of frame_bytes bytes across every boundary between two pushes"""
    total = int(sum(lens))
    bits = hm.draw_stream(rng, total).tolist()
    at = 0
    for n in lens[:-1]:
        at += int(n)
        fb = frame_bits(rng.integers(0, 256, frame_bytes, dtype=np.uint8).tobytes(), 2, 1)
        a = at - len(fb) // 2
        if a >= 0 and a + len(fb) <= total:
            bits[a:a + len(fb)] = fb
    inv, nrzi, des = hx.LINE_CONFIGS[line]
    return hx.line_encode(bits, inv, nrzi, des)


# ---- 1. ragged streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["dev", "host"])
def test_ragged_streams_with_zero_count_pushes_mid_frame(via):
    """counts 0, 1 and 9,000 (two tile seams) in one push, rotated over three more: every stream sits out a push, streams 0 and 2
    with a frame open across it (a frame straddles symbol 9,000 of each), which stream 2's next push completes"""
    cfg = (1, 50, FIX, "nrzi+g3ruh")
    rng = np.random.default_rng(11)
    rot = [(0, 1, 9000), (9000, 0, 1), (1, 9000, 0), (0, 1, 9000)]
    per_stream = [[r[c] for r in rot] for c in range(3)]
    sy = [plant(rng, [n for n in per_stream[c] if n], "nrzi+g3ruh") for c in range(3)]
    rx = make_rx(3, cfg)
    singles, models, at, seen = [Single(cfg) for _ in range(3)], [model(cfg) for _ in range(3)], [0, 0, 0], 0
    for counts in rot:
        buf = np.zeros((3, 9000), np.float32)
        for c in range(3):
            buf[c, :counts[c]] = sy[c][at[c]:at[c] + counts[c]]
            at[c] += counts[c]
        got = feed(rx, buf, counts, via)
        assert got == expect(singles, buf, counts)
        assert got == expect(models, buf, counts)
        seen += sum(len(f) for f in got[0])
    assert seen > 100 and sum(s[2] for s in got[1]) > 0


def test_null_counts_mean_n_cap_for_every_stream():
    cfg = (1, 50, 0, "nrzi")
    rng = np.random.default_rng(12)
    sy = np.stack([plant(rng, [3000, 3000], "nrzi") for _ in range(3)])
    rx, singles = make_rx(3, cfg), [Single(cfg) for _ in range(3)]
    for a in (0, 3000):
        got = feed(rx, sy[:, a:a + 3000], None)
        assert got == expect(singles, sy[:, a:a + 3000], None)
    assert got[2] == [6000] * 3 and sum(s[0] for s in got[1]) > 30


# ---- 2. what lies at and beyond a stream's count is never read ----------------------------------------------------------------------
def test_unread_tails_and_counts_beyond_n_cap():
    cfg = (1, 50, FIX, "plain")
    rng = np.random.default_rng(13)
    n_cap, counts = 600, [600, 200, 0]
    base = np.stack([hx.line_encode(hm.draw_stream(rng, n_cap)) for _ in range(3)])
    valid = hx.line_encode((FLAG + frame_bits(b"tail of another stream", 1, 1) * 3)[:n_cap])
    results = []
    for fill in ("zeros", "nan", "frames"):
        buf = base.copy()
        for c in range(3):
            k = counts[c]
            buf[c, k:] = {"zeros": 0.0, "nan": np.nan}.get(fill, 0.0)
            if fill == "frames":
                buf[c, k:] = valid[:n_cap - k]
        rx = make_rx(3, cfg)
        results.append([feed(rx, buf, counts), feed(rx, buf, counts)])
    assert results[0] == results[1] == results[2]
    assert results[0][1][2] == [1200, 400, 0] and len(results[0][0][0][0]) > 0
    # a count above n_cap is n_cap: the buffer really is that large, so nothing lies outside it
    a, b = make_rx(3, cfg), make_rx(3, cfg)
    assert feed(a, base, [601, 10 ** 12, 2 ** 63]) == feed(b, base, [600, 600, 600]) == feed(make_rx(3, cfg), base, None)


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------------------
def test_one_stream_changes_only_its_own_frames_counters_and_arena():
    cfg = (1, 50, FIX, "nrzi+g3ruh")
    rng = np.random.default_rng(14)
    sy = np.stack([plant(rng, [1500], "nrzi+g3ruh") for _ in range(4)])
    other = sy.copy()
    other[2] = plant(rng, [1500], "nrzi+g3ruh")
    out = []
    for x in (sy, other):
        rx = make_rx(4, cfg)
        snap = feed(rx, x)
        arena = rx.frame_bytes()
        assert len(arena) % 4 == 0
        out.append((snap, arena.reshape(4, -1).copy(), rx.frames()))
    (s0, a0, f0), (s1, a1, f1) = out
    for c in (0, 1, 3):
        assert s0[0][c] == s1[0][c] and s0[1][c] == s1[1][c] and np.array_equal(a0[c], a1[c])
        assert np.array_equal(f0[f0["stream"] == c], f1[f1["stream"] == c])
    assert s0[0][2] != s1[0][2] and not np.array_equal(a0[2], a1[2])
    # every frame lies in its own stream's region
    region = a0.shape[1]
    assert all(int(r["start"]) // region == int(r["stream"]) or int(r["len"]) == 0 for r in f0) and len(f0) > 20


# ---- 4. every configuration ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", list(hx.LINE_CONFIGS))
@pytest.mark.parametrize("flags", [0, KEEP, FIX, KEEP | FIX])
def test_every_configuration(flags, line):
    cfg = (1, 40, flags, line)
    rng = np.random.default_rng(15)
    sy = np.stack([plant(rng, [1300, 1200], line, 20) for _ in range(3)])
    rx, singles, models = make_rx(3, cfg), [Single(cfg) for _ in range(3)], [model(cfg) for _ in range(3)]
    for a, b in ((0, 1300), (1300, 2500)):
        buf = np.ascontiguousarray(sy[:, a:b])
        got = feed(rx, buf)
        assert got == expect(singles, buf, None)
        assert got == expect(models, buf, None)
    stats = np.array(got[1])
    assert stats[:, 0].sum() > 10
    if not flags & KEEP:                        # the drawn streams hold frames with one bit flipped
        assert stats[:, 1].sum() > 0
        assert (stats[:, 2].sum() > 0) == bool(flags & FIX)


# ---- 5. the carry differs per stream -------------------------------------------------------------------------------------------------
def test_carry_differs_per_stream():
    """stream 0 holds the frame of max_size - 1 stuffed all-ones bytes — the carry bound — open across three pushes while its
    neighbours close short frames in every push; then a gap longer than hdlc_reach in stream 1 only"""
    mx = 40
    cfg = (1, mx, KEEP, "plain")
    rx = make_rx(3, cfg)
    tile, carry = rx.dims()
    M = 8 * mx + 1
    assert carry == M + (M - 1) // 5 + 16 and tile == 4096
    long_frame = FLAG + stuff(bytes_to_bits(b"\xff" * (mx - 1))) + FLAG
    n = 140
    assert 2 * n < len(long_frame) - 8 < 3 * n
    short = lambda k: (FLAG + frame_bits(bytes([k + 1] * 5), 1, 1, with_crc=False) + FLAG * 20)[:n]
    rows = [long_frame + [0, 1] * n, sum((short(k) for k in range(4)), []), sum((short(k + 4) for k in range(4)), [])]
    gap = [0, 1] * 260                          # no flag for longer than hdlc_reach(40) = 393 bits
    rows[1] = rows[1] + gap + FLAG + frame_bits(b"after the gap", 1, 1, with_crc=False)
    total = max(len(r) for r in rows)
    total += -total % n
    sy = np.stack([hx.line_encode(r + [0, 1] * total)[:total] for r in rows])
    singles, models = [Single(cfg) for _ in range(3)], [model(cfg) for _ in range(3)]
    per_push = []
    for a in range(0, total, n):
        buf = np.ascontiguousarray(sy[:, a:a + n])
        got = feed(rx, buf)
        assert got == expect(singles, buf, None)
        assert got == expect(models, buf, None)
        per_push.append([len(f) for f in got[0]])
    assert [p[0] for p in per_push[:3]] == [0, 0, 1] and all(p[1] >= 1 and p[2] >= 1 for p in per_push[:3])
    assert got[1][0][0] == 1 and got[1][1][0] >= 5 and got[1][2][0] >= 4


# ---- 6. stream counts at the edges of the mapping ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases():
    """8 base streams of 64 .. 300 symbols in two pushes and what the single-stream handles make of them"""
    cfg = (1, 40, FIX, "nrzi+g3ruh")
    rng = np.random.default_rng(16)
    lens = [64, 65, 100, 128, 191, 256, 299, 300]
    sy = np.zeros((8, 2, 300), np.float32)
    want = []
    for k, n in enumerate(lens):
        s = plant(rng, [n, n], "nrzi+g3ruh", 12)
        sy[k, 0, :n], sy[k, 1, :n] = s[:n], s[n:]
        one = Single(cfg)
        want.append([(one.push(s[:n]), one.stats()), (one.push(s[n:]), one.stats())])
    assert sum(len(w[0][0]) + len(w[1][0]) for w in want) > 3
    return cfg, lens, sy, want


@pytest.mark.parametrize("n", [1, 2, 64, 65, 4096])
def test_stream_counts_at_the_edges_of_the_mapping(bases, n):
    cfg, lens, sy, want = bases
    rx = make_rx(n, cfg)
    pick = [(c * 5 + n) % 8 for c in range(n)]
    counts = [lens[k] for k in pick]
    for push in (0, 1):
        frames, stats, consumed = feed(rx, sy[pick, push, :], counts)
        for c in range(n):
            assert frames[c] == want[pick[c]][push][0] and stats[c] == want[pick[c]][push][1], (c, push)
        assert consumed == [(push + 1) * k for k in counts]


def test_one_stream_equals_the_single_stream_handles_record_for_record():
    cfg = (1, 50, FIX, "nrzi+g3ruh")
    rng = np.random.default_rng(17)
    s = plant(rng, [5000, 4000], "nrzi+g3ruh")
    rx, one = make_rx(1, cfg), Single(cfg)
    for a, b in ((0, 5000), (5000, 9000)):
        feed(rx, s[None, a:b])
        one.push(s[a:b])
        got, want = rx.frames(), one.df.frames()
        assert len(got) == len(want) > 10
        for k in ("pos", "start", "len", "flags"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(rx.frame_bytes(), one.df.frame_bytes())
        assert tuple(rx.stats()[0]) == one.stats()


def test_a_workspace_grown_once_serves_smaller_pushes_in_both_handle_families():
    """pushes of 10, 9,000, 0 and 10 symbols: the workspace both handle families now plan in one place (hdlc_plan, HdlcCore) grows
    over two tile seams, sits out a push and is reused far larger than the last push needs.  plant() finds no room for a frame
    around pushes of 10 symbols, so one is laid by hand: its last bit is bit 8,999, which the scrambler's 17 bits of delay put 6
    symbols into the last push, and it is open across the empty one."""
    cfg = (1, 50, FIX, "nrzi+g3ruh")
    rng = np.random.default_rng(19)
    lens = [10, 9000, 0, 10]
    bits = hm.draw_stream(rng, sum(lens)).tolist()
    fb = frame_bits(rng.integers(0, 256, 30, dtype=np.uint8).tobytes(), 2, 1)
    bits[9000 - len(fb):9000] = fb
    s = hx.line_encode(bits, *hx.LINE_CONFIGS[cfg[3]])
    rx, one, mod = make_rx(1, cfg), Single(cfg), model(cfg)
    at, per_push, want = 0, [], []
    for n in lens:
        x = s[at:at + n]
        at += n
        if n:
            feed(rx, x[None, :])
            one.push(x)
        else:                                   # both handles are told of the empty push: it has no frames
            rx.push_dev(0, 0, 0)
            one.df.push(np.zeros(0, np.uint8))
        got, ref = rx.frames(), one.df.frames()
        assert len(got) == len(ref)
        for k in ("pos", "start", "len", "flags"):
            assert np.array_equal(got[k], ref[k]), (n, k)
        assert np.array_equal(rx.frame_bytes(), one.df.frame_bytes()), n
        assert tuple(int(v) for v in rx.stats()[0]) == one.stats(), n
        per_push.append(rx.result()[0])
        want.append(mod.push(x))
    assert per_push == want and tuple(int(v) for v in rx.stats()[0]) == mod.stats()
    assert [len(p) for p in per_push][::2] == [0, 0] and len(per_push[1]) > 10 and len(per_push[3]) == 1
    assert len(per_push[3][0][1]) == 30 and int(rx.consumed()[0]) == sum(lens)


def test_launch_count_does_not_depend_on_streams_or_symbols(bases):
    """seven launches and one profiling bracket for 1 and for 4,096 streams, for empty and for full streams"""
    cfg, lens, sy, _ = bases
    seen = set()
    for n, counts in ((1, [300]), (1, [0]), (4096, [300] * 4096), (4096, [0] * 4096), (4096, None)):
        rx = make_rx(n, cfg)
        rx.set_profiling(True)
        d = torch.from_numpy(np.ascontiguousarray(sy[[c % 8 for c in range(n)], 0, :])).cuda()
        dc = torch.from_numpy(np.asarray(counts, np.int64)).cuda() if counts is not None else None
        l0 = launches()
        rx.push_dev(d.data_ptr(), 300, 300, dc.data_ptr() if dc is not None else None, stream0())
        seen.add((launches() - l0, rx.profile()[1]))
        rx.frames()
    assert seen == {(7, 1)}


# ---- 7. the chain it exists for ----------------------------------------------------------------------------------------------------------
def test_symbol_sync_feeds_the_receiver_without_a_host_read():
    x = hx.chain_samples()
    N, n = x.shape
    cuts = [hx.CHAIN_CUT, n - hx.CHAIN_CUT]
    _, mframes, mstats = hx.chain_model(x, cuts)
    assert all(sum(len(p[c]) for p in mframes) >= 1 for c in range(N))          # the equality below is not vacuous
    ss = rr.SymbolSync(hx.CHAIN_SPS, 0.0, hx.CHAIN_TAPS, N)
    rx = rr.HdlcReceiver(N, 1, hx.CHAIN_MAX_SIZE, nrzi=True, descrambler=hx.G3RUH)
    # the path that downloads the counts in between
    ss2 = rr.SymbolSync(hx.CHAIN_SPS, 0.0, hx.CHAIN_TAPS, N)
    rx2 = rr.HdlcReceiver(N, 1, hx.CHAIN_MAX_SIZE, nrzi=True, descrambler=hx.G3RUH)
    dx = torch.from_numpy(x).cuda()
    s, at = stream0(), 0
    for i, k in enumerate(cuts):
        win = dx[:, at:at + k].contiguous()
        syms = torch.zeros((N, k), dtype=torch.float32, device="cuda")
        ss.push_dev(win.data_ptr(), k, k, syms.data_ptr(), None, k, s)
        rx.push_dev(syms.data_ptr(), k, k, ss.counts_dev(), s)                  # nothing read by the host in between
        got = rx.result()
        assert got == mframes[i]
        syms2 = torch.zeros((N, k), dtype=torch.float32, device="cuda")
        ss2.push_dev(win.data_ptr(), k, k, syms2.data_ptr(), None, k, s)
        counts = [int(v) for v in ss2.produced()]
        assert feed(rx2, syms2.cpu().numpy(), counts, "host")[0] == got
        at += k
    assert [tuple(int(v) for v in r) for r in rx.stats()] == mstats == [(3, 0, 0)] * N
    assert [int(v) for v in rx.consumed()] == [int(v) for v in rx2.consumed()]


# ---- 8. loopback with the framer -------------------------------------------------------------------------------------------------------
def test_loopback_with_the_framer():
    rng = np.random.default_rng(18)
    framer = lambda: rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
    packets = [[rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8).tobytes() for _ in range(3 + c)] for c in range(4)]
    # (one more packet behind them: the scrambler's register keeps the last 17 bits of a push)
    sy = [framer().push(p + [b"flush"]) for p in packets]
    n_cap = max(len(s) for s in sy)
    buf = np.zeros((4, n_cap), np.float32)
    for c, s in enumerate(sy):
        buf[c, :len(s)] = s
    rx = rr.HdlcReceiver(4, 1, 50, nrzi=True, descrambler=hx.G3RUH)
    frames, stats, consumed = feed(rx, buf, [len(s) for s in sy])
    for c in range(4):
        assert [f[1] for f in frames[c]][:len(packets[c])] == packets[c] and not any(f[2] for f in frames[c])
        assert stats[c][1:] == (0, 0)
    assert consumed == [len(s) for s in sy]


# ---- 9. seeded fuzz ----------------------------------------------------------------------------------------------------------------------
def fuzz_symbols(rng, n, line):
    inv, nrzi, des = hx.LINE_CONFIGS[line]
    out = hx.line_encode(hm.draw_stream(rng, n), inv, nrzi, des) * rng.uniform(0.1, 3.0, n).astype(np.float32)
    k = rng.integers(0, n, max(n // 200, 1))
    out[k] = rng.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32), len(k))
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65])
def test_seeded_fuzz(n):
    rng = np.random.default_rng(4000 + n)
    line = list(hx.LINE_CONFIGS)[int(rng.integers(0, 4))]
    cfg = (int(rng.integers(0, 4)), int(rng.integers(8, 60)), int(rng.integers(0, 4)), line)
    rx, singles = make_rx(n, cfg), [Single(cfg) for _ in range(n)]
    caps = [int(rng.integers(1, 900)) for _ in range(int(rng.integers(3, 7)))]
    counts = [[0 if rng.random() < 0.25 else int(rng.integers(0, cap + 1)) for _ in range(n)] for cap in caps]
    # every stream is one drawn stream, cut where the counts say
    sy = [fuzz_symbols(rng, max(sum(k[c] for k in counts), 1), line) for c in range(n)]
    at, seen = [0] * n, 0
    for cap, k in zip(caps, counts):
        buf = rng.uniform(-1, 1, (n, cap)).astype(np.float32)          # (what lies beyond a count is noise nobody reads)
        for c in range(n):
            buf[c, :k[c]] = sy[c][at[c]:at[c] + k[c]]
            at[c] += k[c]
        got = feed(rx, buf, k)
        assert got == expect(singles, buf, k), cfg
        seen += sum(len(f) for f in got[0])
    assert seen > 0 and any(0 in k for k in counts)


# ---- 10. refusals and the fetch contracts ----------------------------------------------------------------------------------------------
def test_refusals_and_fetch_contracts():
    cfg = (1, 50, 0, "plain")
    rx = make_rx(3, cfg)
    L = rr.lib()
    d = torch.zeros(3 * 64, dtype=torch.float32, device="cuda")
    l0 = launches()
    for args, msg in (((d.data_ptr(), 63, 64), "hdlc receiver: stride shorter than n_cap"), ((0, 64, 64), "hdlc receiver: null symbols"),
                      ((d.data_ptr(), 2 ** 29, 2 ** 29), "hdlc receiver: more than 2\\^30 symbols in one push")):
        with pytest.raises(ValueError, match=msg):
            rx.push_dev(*args)
    with pytest.raises(RuntimeError, match="HdlcReceiver delivers frames"):
        rx.work(np.zeros(8, np.float32), 8)
    assert launches() == l0
    sy = np.stack([hx.line_encode(FLAG + frame_bits(bytes([c + 1] * 9), 1, 1) * 4) for c in range(3)])
    frames, stats, consumed = feed(rx, sy)
    assert [len(f) for f in frames] == [4, 4, 4] and consumed == [sy.shape[1]] * 3
    total = C.c_size_t(0)
    assert L.rr_hdlc_receiver_frames(rx._h, None, 0, C.byref(total)) == 0 and total.value == 12          # cap == 0 only counts
    part = np.zeros(5 + 1, rr.HDLC_STREAM_FRAME)
    part["pos"][5] = 12345
    assert L.rr_hdlc_receiver_frames(rx._h, part.ctypes.data_as(C.c_void_p), 5, C.byref(total)) == 0 and total.value == 12
    assert np.array_equal(part[:5], rx.frames()[:5]) and part["pos"][5] == 12345                         # truncated at cap
    one = np.zeros(2, np.uint64)
    one[1] = 99
    assert L.rr_hdlc_receiver_consumed(rx._h, one.ctypes.data_as(C.c_void_p), 1, C.byref(total)) == 0
    assert total.value == 3 and one.tolist() == [sy.shape[1], 99]
    assert L.rr_hdlc_receiver_frames(rx._h, None, 3, C.byref(total)) != 0 and "null argument" in rr.last_error()
    p, nbytes = rx.bytes_dev()
    assert p and nbytes == len(rx.frame_bytes()) and nbytes % 3 == 0
    order = rx.frames()
    assert np.array_equal(order, np.sort(order, order=["stream", "pos"]))
    # an empty push: no frames, no arena, every state alone
    l0 = launches()
    rx.push_dev(0, 0, 0)
    assert launches() == l0 and rx.bytes_dev() == (None, 0) and len(rx.frames()) == 0 and len(rx.frame_bytes()) == 0
    assert snapshot(rx)[1:] == (stats, consumed)
    assert feed(rx, sy)[0] == [[(p + sy.shape[1], b, f) for p, b, f in fr] for fr in frames]
