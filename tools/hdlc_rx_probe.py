#!/usr/bin/env python3
"""rr_hdlc_receiver (N symbol streams to checked frames in seven launches) against the path it replaces, built from the unchanged
single-stream blocks; same process, same box, interleaved, the symbols resident in HBM.

    tools/hdlc_rx_probe.py [--steps 5] [--warmup 1] [--out profiles/hdlc_rx_probe.md] [--shapes 0,1,2,3]

Every stream holds looped-back frames: packets through rr_hdlc_framer(FCS | G3RUH | NRZI | SYMBOLS), back to back, as in
tools/hdlc_probe.py.  Shapes: 4,096 x 3,150 symbols (one 16,384-sample window at 5.2 sps; packets of 64 bytes), 256 x 770,000,
32 x 770,000 and 1 x 1,000,000 (packets of 256 bytes).  Per shape, in turn (R, B, C, R, ...):
  (R) one rr_hdlc_receiver_push_dev with the counts on the device plus rr_hdlc_receiver_frames behind it
  (B) the path it replaces: the download of the N counts (what rr_symbol_sync_produced does), then per stream rr_bit_decoder ->
      rr_hdlc_deframer_push_dev -> rr_hdlc_frames.  ONE decoder and ONE deframer handle take the streams in turn: their launches,
      downloads and waits are those of N handle pairs, and 8,192 handles with a HIP stream each are not created for a measurement
  (C) rr_bit_decoder over all N n symbols in one call: the packet-side yardstick
Reported: the median ms with the interquartile range, kernel launches per step, frames per push, B / R.
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

G3RUH = (0x21, 0, 16)
SHAPES = ((4096, 3150, 64), (256, 770_000, 256), (32, 770_000, 256), (1, 1_000_000, 256))


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def looped_back(rng, n, L):
    """n symbols of back-to-back frames of L random bytes (the last one cut)"""
    P = n // (8 * (L + 2)) + 2
    fr = rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
    sy = fr.push_buffer(rng.integers(0, 256, P * L, dtype=np.uint8), (np.arange(P) * L).astype(np.uintp), np.full(P, L, np.uintp))
    assert len(sy) >= n
    return torch.from_numpy(np.ascontiguousarray(sy[:n])).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdlc_rx_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    rows = []
    for N, n, L in [SHAPES[int(k)] for k in a.shapes.split(",")]:
        sym = looped_back(rng, n, L).repeat(N, 1).contiguous()               # every stream the same symbols: the work is per stream
        counts = torch.full((N,), n, dtype=torch.int64, device="cuda")
        rx = rr.HdlcReceiver(N, 0, 4096, nrzi=True, descrambler=G3RUH)
        dec, dfr = rr.BitDecoder(nrzi=True, descrambler=G3RUH), rr.HdlcDeframer(0, 4096, 0)
        bits = torch.empty(n, dtype=torch.uint8, device="cuda")
        allbits = torch.empty(N * n, dtype=torch.uint8, device="cuda")
        times = {"R": [], "B": [], "C": []}
        nl, frames = {}, {}
        for it in range(a.warmup + a.steps):
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                if k == "R":
                    rx.push_dev(sym.data_ptr(), n, n, counts.data_ptr())
                    frames[k] = len(rx.frames())
                elif k == "B":
                    got = counts.cpu()
                    frames[k] = 0
                    for c in range(N):
                        m = int(got[c])
                        dec.work_dev(sym[c].data_ptr(), m, bits.data_ptr(), m)
                        dfr.push_dev(bits.data_ptr(), m)
                        frames[k] += len(dfr.frames())
                else:
                    dec.work_dev(sym.data_ptr(), N * n, allbits.data_ptr(), N * n)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                nl[k] = launches() - l0
        row = {"streams": N, "symbols_per_stream": n, "packet_bytes": L, "frames_R": frames["R"], "frames_B": frames["B"],
               "launches_R": nl["R"], "launches_B": nl["B"]}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
        row["B_over_R"] = round(row["B_ms"] / row["R_ms"], 2)
        row["R_over_C"] = round(row["R_ms"] / row["C_ms"], 2)
        row["R_Msym_per_s"] = round(N * n / (row["R_ms"] * 1e-3) / 1e6, 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del rx, dec, dfr, sym, bits, allbits
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_hdlc_receiver_create: N symbol streams to checked frames, the symbols resident in HBM\n\n"
                f"`tools/hdlc_rx_probe.py --steps {a.steps} --warmup {a.warmup} --shapes {a.shapes}` on {dev}; host-timed, synchronised,\n"
                "median over the steps (interquartile range in brackets).  R = one rr_hdlc_receiver_push_dev with the counts on the\n"
                "device plus rr_hdlc_receiver_frames.  B = the path it replaces: the counts downloaded, then per stream rr_bit_decoder ->\n"
                "rr_hdlc_deframer_push_dev -> rr_hdlc_frames (one handle pair takes the streams in turn: the launches, downloads and\n"
                "waits of N pairs).  C = rr_bit_decoder over all the symbols in one call, the yardstick.  Every stream holds the same\n"
                "looped-back frames; frames per push counts all streams.\n\n"
                "| streams x symbols | frames per push (R / B) | R ms | R launches | R Msym/s | B ms | B launches | C ms | B / R | R / C |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['streams']:,} x {r['symbols_per_stream']:,} | {r['frames_R']:,} / {r['frames_B']:,} | {r['R_ms']} ({r['R_iqr_ms']}) | "
                    f"{r['launches_R']} | {r['R_Msym_per_s']} | {r['B_ms']} ({r['B_iqr_ms']}) | {r['launches_B']:,} | "
                    f"{r['C_ms']} ({r['C_iqr_ms']}) | {r['B_over_R']} | {r['R_over_C']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
