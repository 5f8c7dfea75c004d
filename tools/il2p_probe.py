#!/usr/bin/env python3
"""rr_il2p_receiver (N symbol streams to IL2P headers in three launches) against the path it replaces, built from the unchanged
single-stream blocks and a host deframer; same process, same box, interleaved, the symbols resident in HBM.

    tools/il2p_probe.py [--steps 5] [--warmup 1] [--out profiles/il2p_probe.md] [--shapes 0,1,2,3]

Contents: "planted" = random symbols with an IL2P frame planted every 2,000 symbols, allowed_diffs 0; "dense" = the same symbols
with allowed_diffs 24, where every position from 23 on carries a tag and a header is delivered every 121 symbols.  Shapes:
4,096 x 3,150 symbols, 256 x 770,000, 32 x 770,000 and 1 x 1,000,000.  Per shape and content, in turn (R, B, C, R, ...):
  (R) one rr_il2p_receiver_push_dev with the counts on the device plus rr_il2p_receiver_headers behind it
  (B) the path it replaces: the download of the N counts (what rr_symbol_sync_produced does), then per stream rr_bit_decoder(
      RR_BITS_INVERT, code = SYNC_WORD) -> rr_bit_tags, the download of the stream's bits, and the chain rule and the header decode
      in numpy on one host core.  ONE decoder handle takes the streams in turn: its launches, downloads and waits are those of N
      handles
  (C) rr_bit_decoder (no correlator) over all N n symbols in one call: the packet-side yardstick
Reported: the median ms with the interquartile range, kernel launches per step, headers per push, B / R.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustradio_amd as rr  # noqa: E402

SYNC_WORD = [1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0]
SHAPES = ((4096, 3150), (256, 770_000), (32, 770_000), (1, 1_000_000))


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def planted(rng, n):
    """n line bits (behind the slicer and the inversion): random, the sync word and 120 random header bits every 2,000"""
    b = rng.integers(0, 2, n).astype(np.uint8)
    for at in range(500, n - 144, 2000):
        b[at:at + 24] = SYNC_WORD
    return b


def host_deframe(bits, pos, diffs):
    """the chain rule over the tags of one stream and the decode of the accepted headers, in numpy -> (K, 15) bytes"""
    acc, free_from, n = [], 0, len(bits)
    pos = pos.astype(np.int64)                # (searchsorted with a Python int would convert a uint64 array on every call)
    while True:
        i = int(np.searchsorted(pos, free_from)) if free_from else 0
        if i >= len(pos) or int(pos[i]) + 121 > n:
            break
        acc.append(int(pos[i]))
        free_from = int(pos[i]) + 121
    if not acc:
        return np.zeros((0, 15), np.uint8)
    idx = np.asarray(acc)[:, None] + 1 + np.arange(120)[None, :]
    x = bits[idx]
    y = x.copy()
    y[:, 4:] ^= x[:, :-4]
    y[:, 9:] ^= x[:, :-9]
    y[:, 4:9] ^= 1
    return np.packbits(y, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "il2p_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    rows = []
    for N, n in [SHAPES[int(k)] for k in a.shapes.split(",")]:
        line = planted(rng, n)
        one = torch.from_numpy(np.where(line > 0, -1.0, 1.0).astype(np.float32)).cuda()        # (the receiver inverts)
        sym = one.repeat(N, 1).contiguous()                                # every stream the same symbols: the work is per stream
        counts = torch.full((N,), n, dtype=torch.int64, device="cuda")
        bits = torch.empty(n, dtype=torch.uint8, device="cuda")
        allbits = torch.empty(N * n, dtype=torch.uint8, device="cuda")
        plain = rr.BitDecoder(invert=True)
        for content, allowed in (("planted", 0), ("dense", 24)):
            rx = rr.Il2pReceiver(N, invert=True, allowed_diffs=allowed)
            dec = rr.BitDecoder(invert=True, code=SYNC_WORD, allowed_diffs=allowed)
            times = {"R": [], "B": [], "C": []}
            nl, headers = {}, {}
            same = None
            for it in range(a.warmup + a.steps):
                for k in times:
                    torch.cuda.synchronize()
                    l0, t0 = launches(), time.perf_counter()
                    if k == "R":
                        rx.push_dev(sym.data_ptr(), n, n, counts.data_ptr())
                        rec = rx.headers()
                        headers[k] = len(rec)
                    elif k == "B":
                        got = counts.cpu()
                        headers[k] = 0
                        for c in range(N):
                            m = int(got[c])
                            dec.work_dev(sym[c].data_ptr(), m, bits.data_ptr(), m)
                            pos, diffs = dec.tags()
                            raw = host_deframe(bits[:m].cpu().numpy(), pos, diffs)
                            headers[k] += len(raw)
                            if it == 0 and c == 0:      # both start their stream here: the two paths' headers of stream 0 are the same
                                same = bool(np.array_equal(rec[rec["stream"] == 0]["raw"], raw))
                    else:
                        plain.work_dev(sym.data_ptr(), N * n, allbits.data_ptr(), N * n)
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
                    nl[k] = launches() - l0
                print(f"# {N} x {n} {content}: step {it} done", file=sys.stderr, flush=True)
            row = {"streams": N, "symbols_per_stream": n, "content": content, "allowed_diffs": allowed, "headers_R": headers["R"],
                   "headers_B": headers["B"], "launches_R": nl["R"], "launches_B": nl["B"],
                   "stream0_raw_equal": same}
            for k in times:
                t = np.asarray(times[k])
                row[k + "_ms"] = round(float(np.median(t)), 4)
                row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
            row["B_over_R"] = round(row["B_ms"] / row["R_ms"], 2)
            row["R_over_C"] = round(row["R_ms"] / row["C_ms"], 2)
            row["R_Msym_per_s"] = round(N * n / (row["R_ms"] * 1e-3) / 1e6, 1)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del rx, dec
        del sym, bits, allbits, plain
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_il2p_receiver_create: N symbol streams to IL2P headers, the symbols resident in HBM\n\n"
                f"`tools/il2p_probe.py --steps {a.steps} --warmup {a.warmup} --shapes {a.shapes}` on {dev}; host-timed, synchronised,\n"
                "median over the steps (interquartile range in brackets).  R = one rr_il2p_receiver_push_dev with the counts on the\n"
                "device plus rr_il2p_receiver_headers.  B = the path it replaces: the counts downloaded, then per stream\n"
                "rr_bit_decoder(RR_BITS_INVERT, code = SYNC_WORD) -> rr_bit_tags, the stream's bits downloaded, the chain rule and the\n"
                "header decode in numpy on one host core (one decoder handle takes the streams in turn: the launches, downloads and\n"
                "waits of N handles).  C = rr_bit_decoder without a correlator over all the symbols in one call, the yardstick.  Every\n"
                "stream holds the same symbols: random, a frame planted every 2,000; dense = the same with allowed_diffs 24, a tag at\n"
                "every position and a header every 121.  Headers per push counts all streams, in the last step (R goes on with its\n"
                "streams from push to push, B's host deframer starts anew: a header across the seam is R's alone); the two paths'\n"
                "headers of stream 0 in the first step are compared byte for byte (stream0_raw_equal in the JSON rows).\n\n"
                "| streams x symbols | content | headers per push (R / B) | R ms | R launches | R Msym/s | B ms | B launches | C ms | B / R | R / C |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['streams']:,} x {r['symbols_per_stream']:,} | {r['content']} | {r['headers_R']:,} / {r['headers_B']:,} | "
                    f"{r['R_ms']} ({r['R_iqr_ms']}) | {r['launches_R']} | {r['R_Msym_per_s']} | {r['B_ms']} ({r['B_iqr_ms']}) | "
                    f"{r['launches_B']:,} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['B_over_R']} | {r['R_over_C']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
