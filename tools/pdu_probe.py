#!/usr/bin/env python3
"""Bursts cut, re-centred and batched on the device (rr_stream_to_pdu_create) against what exists without it, same box, interleaved.

    tools/pdu_probe.py [--steps 10] [--warmup 2] [--out profiles/pdu_probe.md]

Two streams, both resident in HBM (the Complex baseband, and the f32 data stream the bursts are cut from):
  the geometry of examples/ax25-9600-wpcr.rs: 50 kS/s, 64 bursts of 25,000 samples of NRZ at 5.2083 samples per symbol, 400 samples
     of silence between them, fed as two pushes of 813,000 samples (a push takes at most 1,024,000); StreamToPdu(max_size
     30,000, tail 50)
  one push of 512,000 samples holding ONE burst of 500,000: the longest PDU the block files (max_size 512,000, tail 50), the worst
     case of Midpointer (one workgroup owns a burst)
Per push the trigger comes from rr_burst_detector over the Complex window, in every variant.  Three ways, in turn (D, A, H, D, ...):
  (D) rr_burst_detector alone: what A and H both contain
  (A) D, then rr_stream_to_pdu_push_dev with RR_PDU_MIDPOINT on the envelope and the data stream, then rr_pdu_records (the wait
      and the download of the records)
  (H) D, then what a user has without the block: rr_burst_edges, StreamToPdu's rules over the edge list on the host, each burst
      downloaded from the data stream (which the caller keeps resident, a burst across two windows included), Midpointer in numpy
      on one host core (mean, partition, two sorts: src/wpcr.rs:62-78)
Reported: the median ms per step (all pushes of the stream) with the interquartile range, A's kernel launches per step, the PDUs
found, and whether A and H agree on the PDUs' positions and lengths and on the offsets (the largest difference: H sums in f32).
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
import rustradio_amd as rr  # noqa: E402

ALPHA, THR = 0.1, 0.3


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def nrz(n, sps, rng):
    lv = rng.choice([-1.0, 1.0], int(n / sps) + 3)
    x = lv[np.floor(np.arange(n) / sps + rng.uniform(0, 1)).astype(np.int64)]
    return (x + 0.3 + rng.normal(0.0, 0.05, n)).astype(np.float32)


def make_stream(nbursts, blen, gap, rng):
    """-> (Complex baseband whose power is 1 inside the bursts, f32 data stream)"""
    n = gap + nbursts * (blen + gap)
    amp = np.zeros(n, np.float32)
    data = (0.05 * rng.standard_normal(n)).astype(np.float32)
    for b in range(nbursts):
        s = gap + b * (blen + gap)
        amp[s:s + blen] = 1.0
        data[s:s + blen] = nrz(blen, 50_000.0 / 9600.0, rng)
    ph = rng.uniform(0, 2 * np.pi, n)
    x = (amp * np.exp(1j * ph) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    return x, data


class HostPdu:
    """StreamToPdu's rules over BurstTagger's edges, the state kept between windows (the closed form of DESIGN.md 4.13)"""

    def __init__(self, max_size, tail):
        self.max_size, self.tail, self.free, self.open, self.w0, self.skip = max_size, tail, 0, None, 0, False

    def window(self, pos, val, n):
        """edges of one window -> [(start, end)] in absolute positions, complete in this window"""
        out = []
        if self.open is not None and self.open[1] is not None:       # waiting for its tail
            r, f = self.open
            if f + self.tail <= self.w0 + n:
                out.append((r, f + self.tail))
                self.open = None
        for p, v in zip(pos, val):
            p = self.w0 + int(p)
            if v:
                self.skip = p < self.free                            # ignored together with its falling edge
                if not self.skip:
                    self.open = (p, None)
            elif self.skip:
                self.skip = False
            elif self.open is not None and self.open[1] is None:
                r = self.open[0]
                if p - r + self.tail <= self.max_size:
                    self.free = p + self.tail
                    if self.free <= self.w0 + n:
                        out.append((r, self.free))
                        self.open = None
                    else:
                        self.open = (r, p)
                else:
                    self.free = r + self.max_size + 1
                    self.open = None
        self.w0 += n
        return out


def host_midpoint(v):
    mean = v.sum(dtype=np.float32) / np.float32(len(v))
    if np.isnan(mean):
        return None
    sel = v > mean
    a, b = np.sort(v[sel]), np.sort(v[~sel])
    if len(a) == 0 or len(b) == 0:
        return None
    low, high = b[len(b) // 2], a[len(a) // 2]
    return np.float32(low + (high - low) / np.float32(2.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdu_probe.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pdu_probe needs a GPU")
    rng = np.random.default_rng(1)
    shapes = [("64 bursts of 25,000 samples at 50 kS/s, two pushes of 813,000", make_stream(64, 25_000, 400, rng), 2, 30_000, 50),
              ("one push of 512,000 samples, one burst of 500,000", make_stream(1, 500_000, 6_000, rng), 1, 512_000, 50)]
    rows = []
    for name, (x, data), npush, max_size, tail in shapes:
        n = len(x) // npush
        assert n * npush == len(x) and n <= rr.PDU_MAX_WINDOW, (len(x), npush)
        d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
        d_data = torch.from_numpy(data).cuda()
        d_env = torch.zeros(len(x), dtype=torch.float32, device="cuda")
        result = {}

        def fresh():
            return rr.BurstDetector(ALPHA, THR), rr.StreamToPdu(THR, max_size, tail, rr.PDU_MIDPOINT), HostPdu(max_size, tail)

        def detect(det, k):
            st, c, p, need = det.work_dev(d_x.data_ptr() + 8 * k * n, n, d_env.data_ptr() + 4 * k * n, n)
            assert p == n

        def step(kind):
            det, pdus, host = fresh()                                # the stream starts over: construction is outside the clock
            torch.cuda.synchronize()
            l0, t0 = launches(), time.perf_counter()
            found = []
            for k in range(npush):
                detect(det, k)
                if kind == "A":
                    pdus.push_dev(d_data.data_ptr() + 4 * k * n, d_env.data_ptr() + 4 * k * n, n)
                    rec = pdus.records()
                    found += [(int(r["stream_pos"]), int(r["len"]), float(r["mid"]) if r["ok"] else None) for r in rec]
                elif kind == "H":
                    pos, val = det.edges()
                    for s, e in host.window(pos, val, n):
                        found.append((s, e - s, host_midpoint(d_data[s:e].cpu().numpy())))
                else:
                    det.sync()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            result[kind] = (found, launches() - l0)
            return dt

        times = {"D": [], "A": [], "H": []}
        for it in range(a.warmup + a.steps):
            for kind in times:
                dt = step(kind)
                if it >= a.warmup:
                    times[kind].append(dt)
        fa, fh = result["A"][0], result["H"][0]
        same = [(s, l) for s, l, _ in fa] == [(s, l) for s, l, _ in fh]
        dmid = max([abs(p[2] - q[2]) for p, q in zip(fa, fh) if p[2] is not None and q[2] is not None] or [0.0]) if same else float("nan")
        row = {"shape": name, "samples": len(x), "pushes": npush, "pdus": len(fa), "pdu_samples": int(sum(l for _, l, _ in fa)),
               "A_launches": result["A"][1], "D_launches": result["D"][1], "A_pdus_equal_H": same, "max_mid_diff": float(dmid)}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
        row["A_minus_D_ms_per_push"] = round((row["A_ms"] - row["D_ms"]) / npush, 4)
        row["H_minus_D_ms_per_push"] = round((row["H_ms"] - row["D_ms"]) / npush, 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d_x, d_data, d_env
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# rr_stream_to_pdu_create: bursts cut, re-centred and batched on the device\n\n"
                f"`tools/pdu_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed steps, synchronised, median over the steps\n"
                "(interquartile range in brackets); a step is every push of the stream on fresh handles.  D = rr_burst_detector alone (part of\n"
                "A and of H), A = D + rr_stream_to_pdu_push_dev with RR_PDU_MIDPOINT + rr_pdu_records, H = D + rr_burst_edges + StreamToPdu's\n"
                "rules on the host + each burst downloaded + Midpointer in numpy on one host core.  No pass mark.\n\n"
                "| stream | samples | pushes | PDUs | PDU samples | D ms | A ms | A launches | H ms | (A - D) per push | (H - D) per push | A PDUs = H PDUs | max mid diff |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['samples']} | {r['pushes']} | {r['pdus']} | {r['pdu_samples']} | {r['D_ms']} ({r['D_iqr_ms']}) | "
                    f"{r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | {r['H_ms']} ({r['H_iqr_ms']}) | {r['A_minus_D_ms_per_push']} | "
                    f"{r['H_minus_D_ms_per_push']} | {'yes' if r['A_pdus_equal_H'] else 'no'} | {r['max_mid_diff']:.3g} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
