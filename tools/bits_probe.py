#!/usr/bin/env python3
"""The fused bit decoder (rr_bit_decoder_create) against what exists without it, same box, interleaved, windows resident
in HBM.

    tools/bits_probe.py [--steps 20] [--warmup 3] [--out profiles/bits_probe.md]

The shape is examples/ax25-9600-rx.rs:195-204: BinarySlicer -> NrziDecode -> Descrambler(0x21, 0, 16) and the HDLC flag
0,1,1,1,1,1,1,0 with no differences allowed as the access code, on random +-1 symbols with noise of sigma 0.2 (one position in
256 carries a tag), at 512,000 samples per call (the reference's ring) and at 1e8.  Three ways over device windows, in turn
(A, B, C, A, ...):
  (A) rr_bit_decoder: one block, bits and tags
  (B) rr_binary_slicer -> rr_nrzi_decode -> rr_descrambler -> rr_correlate_access_code_tag through device buffers: the four
      single GPU blocks, the same kernel launched four times
  (C) rr_quaddemod on a Complex window of the same sample count: the yardstick of the earlier probes, one pass at 12 B per
      sample against A's 5
One step = one work_dev() call per block over the whole window, synchronised, handles kept (every step is the next window of
one stream).  Reported: the median ms per step with the interquartile range, kernel launches per call, the share of 8 TB/s
on A's compulsory bytes (5 n: 4 in, 1 out) for A and B and on C's own 12 n for C, whether A's bits and tags equal B's, and
whether A is slower than B or than C: it is when the medians differ by at least the sum of the two interquartile ranges.
The tags are not fetched inside a step, as a graph that only stores the bits would not; what rr_bit_tags costs on top (two small
launches that close the gaps between the tiles' entries, and the download) is timed separately, median of five.
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
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def symbols(n):
    """random +-1 with noise of sigma 0.2, made on the device"""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 0.2 * torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    x += 2.0 * torch.randint(0, 2, (n,), device="cuda", generator=g).to(torch.float32) - 1.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bits_probe.md"))
    a = ap.parse_args()
    rows = []
    for name, n in (("512,000 samples per call (the reference's ring)", 512_000), ("1e8 samples per call", 100_000_000)):
        x = symbols(n)
        z = torch.view_as_complex(torch.stack([x, x.flip(0)], dim=1).contiguous())      # C's window: n Complex samples
        ya, yb, b1, b2, b3 = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(5))
        yc = torch.empty(n, dtype=torch.float32, device="cuda")
        dec = rr.BitDecoder(nrzi=True, descrambler=G3RUH, code=FLAG)
        sl, nz, ds, cac = rr.BinarySlicer(), rr.NrziDecode(), rr.Descrambler.g3ruh(), rr.CorrelateAccessCodeTag(FLAG, 0)
        qd = rr.QuadratureDemod(1.0)

        def step(k):
            if k == "A":
                return dec.work_dev(x.data_ptr(), n, ya.data_ptr(), n)[2]
            if k == "B":
                p = sl.work_dev(x.data_ptr(), n, b1.data_ptr(), n)[2]
                p = nz.work_dev(b1.data_ptr(), p, b2.data_ptr(), n)[2]
                p = ds.work_dev(b2.data_ptr(), p, b3.data_ptr(), n)[2]
                return cac.work_dev(b3.data_ptr(), p, yb.data_ptr(), n)[2]
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
        fetch = []                                                                 # what asking for the tags costs afterwards
        for it in range(5):
            step("A")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.tags()
            fetch.append((time.perf_counter() - t0) * 1e3)
            step("B")                                                              # (B's stream stays in step with A's)
        torch.cuda.synchronize()
        pa, da = dec.tags()                                                        # every step is the next window of each stream
        pb, db = cac.tags()
        same = bool(torch.equal(ya, yb)) and np.array_equal(pa, pb) and np.array_equal(da, db)
        ntags = len(pa)
        del dec, sl, nz, ds, cac, qd
        row = {"shape": name, "n": n, "A_bit_equals_B": same, "tags_last_call": ntags, "A_tags_fetch_ms": round(float(np.median(fetch)), 4)}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
            row[k + "_launches"] = nl[k]
            row[k + "_of_8TBps"] = round((12 if k == "C" else 5) * n / (row[k + "_ms"] * 1e-3) / 8e12, 4)
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["C_over_A"] = round(row["C_ms"] / row["A_ms"], 2)
        row["A_slower_than_B"] = bool(row["A_ms"] - row["B_ms"] >= row["A_iqr_ms"] + row["B_iqr_ms"])
        row["A_slower_than_C"] = bool(row["A_ms"] - row["C_ms"] >= row["A_iqr_ms"] + row["C_iqr_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, z, ya, yb, b1, b2, b3, yc
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_bit_decoder_create: BinarySlicer -> NrziDecode -> Descrambler(G3RUH) -> CorrelateAccessCodeTag(HDLC flag) as one block\n\n"
                f"`tools/bits_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed work_dev() calls, synchronised,\n"
                "median over the steps (interquartile range in brackets).  A = rr_bit_decoder (bits and tags), B = rr_binary_slicer ->\n"
                "rr_nrzi_decode -> rr_descrambler -> rr_correlate_access_code_tag through device buffers, C = rr_quaddemod on a Complex\n"
                "window of the same sample count (the yardstick: one pass at 12 B per sample).  Share of 8 TB/s: A and B on A's compulsory\n"
                "5 n bytes, C on its own 12 n.  A counts as slower than another way when its median is behind by at least the sum of the\n"
                "two interquartile ranges.  Tags fetch: one rr_bit_tags call after a step (gather launches and download), not part of a step.\n\n"
                "| shape | A ms | launches | A of 8 TB/s | B ms | launches | B of 8 TB/s | C ms | launches | C of 8 TB/s | B / A | C / A | A = B | A slower than B | A slower than C | tags of the last call | tags fetch ms |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | {r['A_of_8TBps']} | {r['B_ms']} ({r['B_iqr_ms']}) | "
                    f"{r['B_launches']} | {r['B_of_8TBps']} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['C_launches']} | {r['C_of_8TBps']} | "
                    f"{r['B_over_A']} | {r['C_over_A']} | {'yes' if r['A_bit_equals_B'] else 'NO'} | "
                    f"{'yes' if r['A_slower_than_B'] else 'no'} | {'yes' if r['A_slower_than_C'] else 'no'} | {r['tags_last_call']} | {r['A_tags_fetch_ms']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
