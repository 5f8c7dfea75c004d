#!/usr/bin/env python3
"""The fused burst detector (rr_burst_detector_create) against what exists without it, same box, interleaved, windows
resident in HBM.

    tools/burst_probe.py [--steps 20] [--warmup 3] [--out profiles/burst_probe.md]

The shape is examples/burst_saver.rs:111-123: ComplexToMag2 -> SinglePoleIirFilter(0.01) -> BurstTagger(1e-3) on noise with
bursts, at 1e8 samples per call and at the reference's ring size (512,000 samples per call).  Three ways over the same device
window, in turn (A, B, C, A, ...):
  (A) rr_burst_detector: one block, envelope and edges
  (B) rr_complex_to_mag2 into a device buffer, then rr_single_pole_iir on it: the unfused pair of GPU blocks (it finds no
      edges: that would be a host pass over the envelope on top)
  (C) rr_quaddemod on the same window: the yardstick — it moves the same compulsory 12 B per sample (8 in, 4 out) in one pass
One step = one work_dev() call of each way over the whole window, synchronised, handles kept (every step is the next window
of one stream).  Reported: the median ms per step with the interquartile range, kernel launches per call, the share of
8 TB/s on the compulsory bytes (12 n), and whether A is slower than B: it is when the medians differ by more than the sum of
the two interquartile ranges in B's favour.
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

ALPHA, THR = 0.01, 1e-3


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def signal(n):
    """noise of sigma 0.003 per component, a burst of amplitude 0.1 in the second quarter of every 100,000 samples; made on the device"""
    g = torch.Generator(device="cuda").manual_seed(1)
    z = 0.003 * torch.randn(2 * n, dtype=torch.float32, device="cuda", generator=g)
    k = torch.arange(n, device="cuda")
    on = ((k % 100_000) >= 25_000) & ((k % 100_000) < 50_000)
    ph = 0.3 * (k % 1_000_000).to(torch.float32)
    z[0::2] += 0.1 * torch.cos(ph) * on
    z[1::2] += 0.1 * torch.sin(ph) * on
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burst_probe.md"))
    a = ap.parse_args()
    rows = []
    for name, n in (("512,000 samples per call (the reference's ring)", 512_000), ("1e8 samples per call", 100_000_000)):
        z = signal(n)
        ya = torch.empty(n, dtype=torch.float32, device="cuda")
        yb = torch.empty(n, dtype=torch.float32, device="cuda")
        yc = torch.empty(n, dtype=torch.float32, device="cuda")
        mid = torch.empty(n, dtype=torch.float32, device="cuda")
        det, m2, iir, qd = rr.BurstDetector(ALPHA, THR), rr.ComplexToMag2(), rr.SinglePoleIirFilter(ALPHA), rr.QuadratureDemod(1.0)

        def step(k):
            if k == "A":
                return det.work_dev(z.data_ptr(), n, ya.data_ptr(), n)[2]
            if k == "B":
                p = m2.work_dev(z.data_ptr(), n, mid.data_ptr(), n)[2]
                return iir.work_dev(mid.data_ptr(), p, yb.data_ptr(), n)[2]
            return qd.work_dev(z.data_ptr(), n, yc.data_ptr(), n)[2]

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
                assert p == n or (k == "C" and p == n - 1), (k, p, n)          # (the demodulator pairs samples: n - 1 outputs)
        same = bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32)))       # every step is the same window of each stream
        nedges = len(det.edges()[0])
        del det, m2, iir, qd
        row = {"shape": name, "n": n, "A_bit_equals_B": same, "edges_last_call": nedges}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
            row[k + "_launches"] = nl[k]
            row[k + "_of_8TBps"] = round(12 * n / (row[k + "_ms"] * 1e-3) / 8e12, 4)
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["A_over_C"] = round(row["A_ms"] / row["C_ms"], 2)
        row["A_slower_than_B"] = bool(row["A_ms"] - row["B_ms"] >= row["A_iqr_ms"] + row["B_iqr_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del z, ya, yb, yc, mid
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_burst_detector_create: ComplexToMag2 -> SinglePoleIirFilter(0.01) -> BurstTagger(1e-3) as one block\n\n"
                f"`tools/burst_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed work_dev() calls, synchronised,\n"
                "median over the steps (interquartile range in brackets).  A = rr_burst_detector (envelope and edges), B =\n"
                "rr_complex_to_mag2 -> rr_single_pole_iir through a device buffer (no edges), C = rr_quaddemod on the same window (the\n"
                "yardstick: the same compulsory 12 B per sample in one pass).  Share of 8 TB/s on those 12 n bytes.  A counts as slower\n"
                "than B when its median is behind by at least the sum of the two interquartile ranges.\n\n"
                "| shape | A ms | launches | A of 8 TB/s | B ms | launches | B of 8 TB/s | C ms | launches | B / A | A / C | A slower than B |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | {r['A_of_8TBps']} | {r['B_ms']} ({r['B_iqr_ms']}) | "
                    f"{r['B_launches']} | {r['B_of_8TBps']} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['C_launches']} | {r['B_over_A']} | {r['A_over_C']} | "
                    f"{'yes' if r['A_slower_than_B'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
