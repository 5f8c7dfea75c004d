#!/usr/bin/env python3
"""Whole-packet clock recovery on the device (rr_wpcr_create) against what exists without it, same box, interleaved.

    tools/wpcr_probe.py [--steps 10] [--warmup 2] [--out profiles/wpcr_probe.md]

Two batches, both resident in HBM:
  64 bursts shaped like 9600-baud AX.25 at 50 kS/s (examples/ax25-9600-wpcr.rs): random NRZ at 5.2083 samples per symbol, three
     samples of smoothing, noise of sigma 0.05, 0.5 s = 25,000 samples each, one sample apart in the buffer
  one burst of 512,000 samples of pure noise: the longest burst the block takes and the most crossings it can have, the worst
     case of the sparse transform (N / 2 bins x C crossings phasors)
Three ways, in turn (A, C, H, A, ...):
  (A) rr_wpcr_process_dev over the batch, then rr_wpcr_results (the wait and the download of the records)
  (C) rr_quaddemod on a Complex window of as many samples: the yardstick of the earlier probes
  (H) what a user has today: the bursts downloaded, then Wpcr::process_one stated in numpy on one host core per burst
      (numpy.fft for the transform, the decision and the picks as array operations), symbols left on the host
Reported: the median ms per step with the interquartile range, A's kernel launches, crossings and phasors of the batch and A's
phasors per second, and whether A's bins equal H's.  The figures have no pass mark.
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


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def nrz(n, sps, rng):
    lv = rng.choice([-1.0, 1.0], int(n / sps) + 3)
    x = lv[np.floor(np.arange(n) / sps + rng.uniform(0, 1)).astype(np.int64)]
    x = np.convolve(x, np.ones(3) / 3.0, mode="same")
    return (x + rng.normal(0.0, 0.05, n)).astype(np.float32)


def host_wpcr(x):
    """Wpcr::process_one (src/wpcr.rs:130-197) as numpy array operations -> (bin or None, symbols)"""
    n = len(x)
    if n < 4:
        return None, None
    s = (x > 0).astype(np.float32)
    d = (s[:-1] - s[1:]) ** 2
    X = np.fft.fft(d)[:len(d) // 2]
    mag = np.abs(X).astype(np.float32)
    if len(mag) < 4:
        return None, None
    thresh = mag[2:].max() * np.float32(0.8)
    hit = np.nonzero((mag[2:-1] > thresh) & (mag[2:-1] > mag[3:]))[0]
    if not len(hit):
        return None, None
    b = int(hit[0]) + 2
    f = np.float32(b) / np.float32(n)
    t = np.float32(0.5) + np.float32(np.angle(X[b])) / np.float32(2 * np.pi)
    p0 = t if t > 0.5 else t + np.float32(1.0)
    fl = np.floor(float(p0) + np.arange(n) * float(f))
    return b, x[np.nonzero(np.diff(np.concatenate([[0.0], fl])) > 0)[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpcr_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    shapes = []
    lens = [25_000] * 64
    starts = [1 + b * 25_001 for b in range(64)]
    x = np.zeros(starts[-1] + lens[-1] + 1, np.float32)
    for s, n in zip(starts, lens):
        x[s:s + n] = nrz(n, 50_000.0 / 9600.0, rng)
    shapes.append(("64 bursts of 25,000 samples, 9600 baud at 50 kS/s", x, starts, lens))
    shapes.append(("1 burst of 512,000 samples of noise", rng.normal(0.0, 1.0, 512_000).astype(np.float32), [0], [512_000]))
    rows = []
    for name, x, starts, lens in shapes:
        n_total = len(x)
        d_x = torch.from_numpy(x).cuda()
        d_s = torch.zeros(n_total, dtype=torch.float32, device="cuda")
        z = torch.view_as_complex(torch.stack([d_x, d_x.flip(0)], dim=1).contiguous())
        yc = torch.empty(n_total, dtype=torch.float32, device="cuda")
        w, qd = rr.Wpcr(samp_rate=50_000.0), rr.QuadratureDemod(1.0)
        host_bins = []

        def step(k):
            if k == "A":
                w.process_dev(d_x.data_ptr(), n_total, starts, lens, None, d_s.data_ptr())
                return w.results()
            if k == "C":
                return qd.work_dev(z.data_ptr(), n_total, yc.data_ptr(), n_total)
            h = d_x.cpu().numpy()
            host_bins[:] = [host_wpcr(h[s:s + n])[0] for s, n in zip(starts, lens)]
            return None

        times = {"A": [], "C": [], "H": []}
        nl = 0
        res = None
        for it in range(a.warmup + a.steps):
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                r = step(k)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                if k == "A":
                    nl, res = launches() - l0, r
        cross = phasors = 0
        for s, n in zip(starts, lens):
            c = int(np.count_nonzero(np.diff((x[s:s + n] > 0).astype(np.int8))))
            cross += c
            phasors += c * ((n - 1) // 2)
        gpu_bins = [int(r["bin"]) if r["ok"] else None for r in res]
        row = {"shape": name, "samples": int(sum(lens)), "crossings": cross, "phasors": phasors, "A_launches": nl,
               "A_bins_equal_H": gpu_bins == host_bins, "valid": int(res["ok"].sum())}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
        row["A_phasors_per_s"] = float(f"{phasors / (row['A_ms'] * 1e-3):.3e}")
        row["A_over_C"] = round(row["A_ms"] / row["C_ms"], 1)
        row["H_over_A"] = round(row["H_ms"] / row["A_ms"], 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del w, qd, d_x, d_s, z, yc
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_wpcr_create: whole-packet clock recovery over a batch of bursts, on the device\n\n"
                f"`tools/wpcr_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed calls, synchronised, median over the steps\n"
                "(interquartile range in brackets).  A = rr_wpcr_process_dev on device buffers + rr_wpcr_results, C = rr_quaddemod on a\n"
                "Complex window of as many samples (the yardstick), H = the bursts downloaded and Wpcr::process_one stated in numpy on one\n"
                "host core.  Phasors = sum over the bursts of crossings x bins, the work of the sparse transform.  No pass mark.\n\n"
                "| batch | samples | crossings | phasors | A ms | launches | A phasors / s | C ms | H ms | A / C | H / A | valid | A bins = H bins |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['samples']} | {r['crossings']} | {r['phasors']:.3e} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | "
                    f"{r['A_phasors_per_s']:.3e} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['H_ms']} ({r['H_iqr_ms']}) | {r['A_over_C']} | {r['H_over_A']} | "
                    f"{r['valid']} | {'yes' if r['A_bins_equal_H'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
