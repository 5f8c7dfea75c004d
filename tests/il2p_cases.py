"""What the rr.Il2pReceiver tests share: the seeded fuzz cases (tests/test_il2p_cpu.py shows on the model that none is empty), what
the model expects of a run of pushes, and the comparison of the device's records with it.  Nothing here touches the GPU library."""
import functools

import numpy as np

import il2p_model as im

FUZZ_SEEDS = tuple(range(40))


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """-> (streams [uint8 bits], pushes [(n_cap, counts)], allowed_diffs, invert): up to 3 streams of up to 20,000 bits, random bits
    with frames planted at gaps of 0 .. 400, 0 .. 3 wrong sync bits in each, a whole sync word inside some headers (its tag is
    dropped when the frame's own is accepted: the first frame of stream 0 always is), random ragged pushes"""
    rng = np.random.default_rng(4100 + seed)
    nstreams, allowed, invert = int(rng.integers(1, 4)), int(rng.integers(0, 4)), bool(rng.integers(2))
    streams = []
    for c in range(nstreams):
        n = int(rng.integers(2000 if c == 0 else 1, 20001))
        bits = rng.integers(0, 2, n).astype(np.uint8)
        at, k = int(rng.integers(0, 401)), 0
        while at + 144 <= n:
            first = (c, k) == (0, 0)
            flips = [] if first else rng.choice(24, int(rng.integers(0, 4)), replace=False).tolist()
            fb = im.frame_bits(im.random_header(rng), flips)
            if first or rng.random() < 0.3:
                o = 24 + int(rng.integers(0, 97))
                fb[o:o + 24] = im.SYNC_WORD
            bits[at:at + 144] = fb
            at += 144 + int(rng.integers(0, 401))
            k += 1
        bits.setflags(write=False)
        streams.append(bits)
    left, pushes = [len(b) for b in streams], []
    while any(left):
        n_cap = int(rng.integers(1, 9001))
        counts = []
        for c in range(nstreams):
            r = rng.random()
            counts.append(min(left[c], 0 if r < 0.15 else n_cap if r < 0.6 else int(rng.integers(0, n_cap + 1))))
        if not any(counts):
            c = next(i for i in range(nstreams) if left[i])
            counts[c] = min(left[c], n_cap)
        left = [l - k for l, k in zip(left, counts)]
        pushes.append((n_cap, counts))
    return streams, pushes, allowed, invert


def record(h, stream):
    """a header of the model as the tuple the device's record compares with"""
    flags = (1 if h["ui"] else 0) | (2 if h["fec"] else 0) | (4 if h["hdrtype1"] else 0)
    return (stream, h["pos"], h["diffs"], h["raw"], h["dst"], h["dst_ssid"], h["src"], h["src_ssid"], flags, h["pid"], h["control"],
            h["payload_size"])


def device_records(rec):
    """rr.IL2P_HEADER[] -> the same tuples"""
    out = []
    for r in rec:
        assert not np.any(r["reserved"])
        out.append((int(r["stream"]), int(r["pos"]), int(r["diffs"]), r["raw"].tobytes(), r["dst"].decode("ascii"), int(r["dst_ssid"]),
                    r["src"].decode("ascii"), int(r["src_ssid"]), int(r["flags"]), int(r["pid"]), int(r["control"]),
                    int(r["payload_size"])))
    return out


def expected(streams, pushes, allowed):
    """the model, per stream over that stream's own windows -> ([records of push k, ascending by (stream, pos)], stats
    [(headers, syncs) per stream], consumed [per stream])"""
    per_push = [[] for _ in pushes]
    stats, consumed = [], []
    for c, bits in enumerate(streams):
        took = [min(k[c], n_cap) for n_cap, k in pushes]
        used = int(sum(took))
        headers, tags = im.run(bits[:used], allowed, [t for t in took if t]) if used else ([], [])
        edges = np.cumsum(took)
        for h in headers:
            per_push[int(np.searchsorted(edges, h["end"], side="right"))].append(record(h, c))
        stats.append((len(headers), len(tags)))
        consumed.append(used)
    return [sorted(p) for p in per_push], stats, consumed


def host_rows(streams, pushes, invert, fill=1.0):
    """per push the (nstreams, n_cap) f32 array of symbols: stream c's next counts[c], the rest `fill` (never read)"""
    at, out = [0] * len(streams), []
    for n_cap, counts in pushes:
        a = np.full((len(streams), n_cap), fill, np.float32)
        for c, k in enumerate(counts):
            k = min(k, n_cap)
            a[c, :k] = im.symbols(streams[c][at[c]:at[c] + k], invert)
            at[c] += k
        out.append(a)
    return out


def even_pushes(streams, size):
    """every stream in pushes of `size` symbols (the last one shorter), all streams of one length"""
    n = len(streams[0])
    assert all(len(s) == n for s in streams)
    return [(min(size, n - at), [min(size, n - at)] * len(streams)) for at in range(0, n, size)]


# ---- the loop-back: rr_fsk_tx (bell202) -> rr_afsk_demod -> rr_symbol_sync -> rr_il2p_receiver ------------------------------------------
LOOP_PREAMBLE, LOOP_TAIL = 240, 48           # alternating bits: the clock recovery locks on them; the tail pushes the last frame through the filters


def loopback_line():
    """-> (line bits uint8[], [the two headers' 15 bytes as sent]): a preamble of alternating bits, two IL2P frames back to back, a tail"""
    rng = np.random.default_rng(1200)
    sent = [im.build_header(), im.random_header(rng)]
    alt = lambda n: [(i & 1) for i in range(n)]
    bits = alt(LOOP_PREAMBLE) + im.frame_bits(sent[0]) + im.frame_bits(sent[1]) + alt(LOOP_TAIL)
    return np.array(bits, np.uint8), sent
