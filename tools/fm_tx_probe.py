#!/usr/bin/env python3
"""The fused FM modulator (rr_fm_tx_create) against what exists without it, same box, interleaved, device-resident windows.

    tools/fm_tx_probe.py [--steps 20] [--warmup 3] [--out profiles/fm_tx_probe.md]

The shape is examples/fm_tx.rs:77-92: RationalResampler(10:1) -> Vco(2 pi 5000 / 480000), at 1e8 output samples per call and
at the reference's ring size (512,000 outputs per call).  Three ways over the same device windows, in turn (A, B, C, A, ...):
  (A) rr_fm_tx: one block
  (B) rr_resampler(10, 1, f32) into a device buffer, then rr_vco on it: the unfused pair of GPU blocks
  (C) rr_resampler(10, 1, 8-byte elements) producing the same number of 8-byte outputs: the yardstick — it moves the same
      output bytes with no arithmetic (this change leaves that block's kernel as it was)
One step = one work_dev() call of each way over the whole window, synchronised, handles kept (every step is the next window
of one stream).  Reported: the median ms per step with the interquartile range, kernel launches per call, the share of
8 TB/s on the algorithmic bytes (4 n_in + 8 n_out), and A's time as a ratio to C's.  No threshold: nobody had measured f64
sincos throughput on this part before.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustradio_amd as rr  # noqa: E402

I, D = 10, 1
K = 2.0 * math.pi * 5000 / 480000


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_tx_probe.md"))
    a = ap.parse_args()
    rows = []
    for name, n_out in (("1e8 outputs per call", 100_000_000), ("512,000 outputs per call (the reference's ring)", 512_000)):
        n_in = n_out * D // I
        audio = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n_in).astype(np.float32)).cuda()
        wide = torch.zeros(2 * n_in, dtype=torch.float32, device="cuda")           # n_in 8-byte elements for (C)
        cap = n_out + 64
        ya = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
        yb = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
        yc = torch.empty(2 * cap, dtype=torch.float32, device="cuda")
        mid = torch.empty(cap, dtype=torch.float32, device="cuda")
        tx, rs, vco, rs8 = rr.FmTx(I, D, K), rr.RationalResampler(I, D, np.float32), rr.Vco(K), rr.RationalResampler(I, D, np.complex64)

        def step(k):
            if k == "A":
                return tx.work_dev(audio.data_ptr(), n_in, ya.data_ptr(), cap)[2]
            if k == "B":
                p = rs.work_dev(audio.data_ptr(), n_in, mid.data_ptr(), cap)[2]
                return vco.work_dev(mid.data_ptr(), p, yb.data_ptr(), cap)[2]
            return rs8.work_dev(wide.data_ptr(), n_in, yc.data_ptr(), cap)[2]

        times = {"A": [], "B": [], "C": []}
        nl = {}
        for it in range(a.warmup + a.steps):
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                p = step(k)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                nl[k] = launches() - l0
                assert p == n_out, (k, p, n_out)
        same = bool(torch.equal(torch.isnan(ya[:2 * n_out]), torch.isnan(yb[:2 * n_out]))) and \
            float((ya[:2 * n_out] - yb[:2 * n_out]).abs().max()) < 1e-6               # (each way's own carried phase: not bit-equal)
        del tx, rs, vco, rs8
        alg = 4 * n_in + 8 * n_out
        row = {"shape": name, "n_in": n_in, "n_out": n_out, "A_equals_B_within_1e-6": same}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
            row[k + "_launches"] = nl[k]
        row["A_of_8TBps"] = round(alg / (row["A_ms"] * 1e-3) / 8e12, 4)
        row["B_of_8TBps"] = round(alg / (row["B_ms"] * 1e-3) / 8e12, 4)             # the same algorithmic bytes; it moves twice as many
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["A_over_C"] = round(row["A_ms"] / row["C_ms"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del audio, wide, ya, yb, yc, mid
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_fm_tx_create: RationalResampler(10:1) -> Vco(2 pi 5000 / 480000) as one block\n\n"
                f"`tools/fm_tx_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed work_dev() calls, synchronised,\n"
                "median over the steps (interquartile range in brackets).  A = rr_fm_tx, B = rr_resampler(f32) -> rr_vco through a\n"
                "device buffer, C = rr_resampler on 8-byte elements producing the same output bytes (the yardstick: no arithmetic).\n"
                "Share of 8 TB/s on the algorithmic bytes 4 n_in + 8 n_out.\n\n"
                "| shape | A ms | launches | A of 8 TB/s | B ms | launches | B of 8 TB/s | C ms | launches | B / A | A / C |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | {r['A_of_8TBps']} | {r['B_ms']} ({r['B_iqr_ms']}) | "
                    f"{r['B_launches']} | {r['B_of_8TBps']} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['C_launches']} | {r['B_over_A']} | {r['A_over_C']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
