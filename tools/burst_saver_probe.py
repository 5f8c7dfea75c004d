#!/usr/bin/env python3
"""Complex bursts cut with pre-roll on the device (rr_burst_saver_create) against what exists without it, same box, interleaved.

    tools/burst_saver_probe.py [--steps 10] [--warmup 2] [--out profiles/burst_saver_probe.md]

The geometry of examples/burst_saver.rs: 50 kS/s, SinglePoleIirFilter alpha 0.01, Delay 3000, tail 5000, max_size 50,000 (one
second of samples), the Complex baseband resident in HBM and fed as pushes of 813,000 samples (a push takes at most 1,024,000)
that hold 32 bursts of 12,000 samples each.  Two ways, in turn (A, H, A, ...):
  (A) rr_burst_saver_push_dev, then rr_pdu_records (the wait and the download of the records); the payloads stay in the arena
  (H) what a user has without the block: rr_burst_detector on the window, rr_burst_edges, the window downloaded, Delay as a numpy
      concatenation with the kept history, and StreamToPdu's rules and the cuts on one host core
Reported: the median ms per step (all pushes of the stream) with the interquartile range, A's kernel launches per step, the PDUs
found and whether A and H agree on their positions and lengths, and on the payload bytes of the first and the last one.
The figures have no pass mark.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rustradio_amd as rr  # noqa: E402
from pdu_probe import HostPdu  # noqa: E402

ALPHA, THR, DELAY, TAIL, MAX_SIZE = 0.01, 0.3, 3000, 5000, 50_000
PUSH, NBURSTS, BLEN = 813_000, 32, 12_000


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def make_stream(npush, rng):
    n = npush * PUSH
    gap = (PUSH - NBURSTS * BLEN) // NBURSTS
    amp = np.zeros(n, np.float32)
    for k in range(npush * NBURSTS):
        s = gap // 2 + k * (BLEN + gap)
        amp[s:s + BLEN] = 1.0
    ph = rng.uniform(0, 2 * np.pi, n)
    return (amp * np.exp(1j * ph) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pushes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burst_saver_probe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("burst_saver_probe needs a GPU")
    x = make_stream(a.pushes, np.random.default_rng(1))
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    d_env = torch.zeros(PUSH, dtype=torch.float32, device="cuda")
    result = {}

    def step(kind):
        saver, det, host = rr.BurstSaver(ALPHA, THR, DELAY, MAX_SIZE, TAIL), rr.BurstDetector(ALPHA, THR), HostPdu(MAX_SIZE, TAIL)
        delayed = np.zeros(0, np.complex64)                  # the delayed stream so far that a PDU may still need
        base = 0                                             # its first position
        hist = np.zeros(DELAY, np.complex64)
        torch.cuda.synchronize()
        l0, t0 = launches(), time.perf_counter()
        found, ends = [], {}
        for k in range(a.pushes):
            if kind == "A":
                saver.push_dev(d_x.data_ptr() + 8 * k * PUSH, PUSH)
                rec = saver.records()
                found += [(int(r["stream_pos"]), int(r["len"])) for r in rec]
                if len(rec) and k in (0, a.pushes - 1):
                    i = 0 if k == 0 else len(rec) - 1
                    ends[k] = saver.pdu(i, rec).tobytes()
            else:
                st, c, p, need = det.work_dev(d_x.data_ptr() + 8 * k * PUSH, PUSH, d_env.data_ptr(), PUSH)
                assert p == PUSH
                pos, val = det.edges()
                w = d_x[2 * k * PUSH:2 * (k + 1) * PUSH].cpu().numpy().view(np.complex64)
                both = np.concatenate([hist, w])
                hist = both[len(both) - DELAY:]
                delayed = np.concatenate([delayed, both[:PUSH]])
                cut = []
                for s, e in host.window(pos, val, PUSH):
                    found.append((s, e - s))
                    cut.append(delayed[s - base:e - base].copy())
                if cut and k in (0, a.pushes - 1):
                    ends[k] = (cut[0] if k == 0 else cut[-1]).tobytes()
                keep = min(len(delayed), MAX_SIZE)           # an open burst holds at most max_size samples
                base += len(delayed) - keep
                delayed = delayed[len(delayed) - keep:]
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        result[kind] = (found, launches() - l0, ends)
        return dt

    times = {"A": [], "H": []}
    for it in range(a.warmup + a.steps):
        for kind in times:
            dt = step(kind)
            if it >= a.warmup:
                times[kind].append(dt)
    fa, fh = result["A"], result["H"]
    row = {"samples": len(x), "pushes": a.pushes, "pdus": len(fa[0]), "pdu_samples": int(sum(l for _, l in fa[0])),
           "A_launches": fa[1], "A_pdus_equal_H": fa[0] == fh[0], "payload_bytes_equal": fa[2] == fh[2] and len(fa[2]) > 0}
    for k in times:
        t = np.asarray(times[k])
        row[k + "_ms"] = round(float(np.median(t)), 4)
        row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
    print(json.dumps(row), flush=True)
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# rr_burst_saver_create: Complex bursts cut with pre-roll on the device\n\n"
                f"`tools/burst_saver_probe.py --steps {a.steps} --warmup {a.warmup} --pushes {a.pushes}` on {dev}; host-timed steps,\n"
                "synchronised, median over the steps (interquartile range in brackets); a step is every push of the stream on fresh\n"
                "handles.  The geometry of examples/burst_saver.rs: 50 kS/s, alpha 0.01, Delay 3000, tail 5000, max_size 50,000, pushes\n"
                "of 813,000 samples with 32 bursts each.  A = rr_burst_saver_push_dev + rr_pdu_records, H = rr_burst_detector +\n"
                "rr_burst_edges + the window downloaded + Delay and the cuts in numpy on one host core.  No pass mark.\n\n"
                "| samples | pushes | PDUs | PDU samples | A ms | A launches | H ms | A PDUs = H PDUs | payload bytes equal |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        f.write(f"| {row['samples']} | {row['pushes']} | {row['pdus']} | {row['pdu_samples']} | {row['A_ms']} ({row['A_iqr_ms']}) | "
                f"{row['A_launches']} | {row['H_ms']} ({row['H_iqr_ms']}) | {'yes' if row['A_pdus_equal_H'] else 'no'} | "
                f"{'yes' if row['payload_bytes_equal'] else 'no'} |\n")
        f.write("\nRow as JSON:\n\n```\n" + json.dumps(row) + "\n```\n")


if __name__ == "__main__":
    main()
