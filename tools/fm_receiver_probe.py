#!/usr/bin/env python3
"""The N-station FM receiver block against what exists without it, same box, interleaved A/B, device-resident input.

    tools/fm_receiver_probe.py [--steps 20] [--warmup 3] [--only ROWKIND]

Per shape two ways to the same audio on the same device window:
  (A) rr_fm_receiver: one block, N audio windows
  (B) rr_fm_multi into a device buffer, then one rr_audio_chain handle per channel on that buffer's windows
      (nchan 1: rr_fm_chain + one rr_audio_chain)
One step = one work_dev() pass of each way over the whole window, in turn (A, B, A, B, ...), synchronised, handles kept;
the median over the timed steps is reported with B's interquartile range, input Msamples/s and the compulsory traffic
(8 B in + nchan x 4 B x I1 I2 / (D1 D2) out per input sample) / time / 8 TB/s.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/fm_receiver_probe.py`.
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
from rustradio_amd import multi  # noqa: E402


def shifted(proto, fs, centres):
    k = np.arange(len(proto))
    return np.stack([(proto.astype(np.complex128) * np.exp(2j * np.pi * f * k / fs)).astype(np.complex64) for f in centres])


def shapes():
    proto = rr.low_pass_complex(multi.CFG4_FS, 100e3, 12.5e3)
    c32 = multi.cfg4_taps(proto, list(multi.shard_channels(32, 1, 0)))
    a400 = rr.low_pass(400e3, 20e3, 4e3)
    rtl = shifted(rr.low_pass_complex(1.024e6, 100e3, 1000.0), 1.024e6, [-15e3, -5e3, 5e3, 15e3])
    a200 = rr.low_pass(200e3, 44.1e3, 500.0)
    # second row: rtl_fm's own audio filter design (44.1 kHz cut-off, 500 Hz transition) at the configs[3] channel rate: 1927 taps
    return [("configs[3] 32ch 463 taps 1:6, audio 241 taps 3:25", c32, (1, 6), a400, (3, 25), 2_400_000),
            ("configs[3] 32ch, rtl_fm audio low_pass(400e3, 44.1e3, 500) 6:25", c32, (1, 6), rr.low_pass(400e3, 44.1e3, 500.0), (6, 25), 2_400_000),
            ("rtl_fm 4ch 2467 taps 25:128, audio 6:25", rtl, (25, 128), a200, (6, 25), 2_400_000),
            ("configs[3] 1ch 1:6, audio 3:25", c32[:1], (1, 6), a400, (3, 25), 2_400_000)]


class Existing:
    """(B): rr_fm_multi (rr_fm_chain for one channel) into [C][mid_cap], then one rr_audio_chain per channel window"""

    def __init__(self, taps, rf, at, au, n, out_cap):
        C = len(taps)
        self.rf = rr.FmMulti(taps, rf[0], rf[1], 1.0) if C > 1 else rr.FmChain(taps[0], rf[0], rf[1], 1.0)
        self.au = [rr.AudioChain(at, au[0], au[1], 0.5) for _ in range(C)]
        self.mid_cap = n * rf[0] // rf[1] + 16
        self.C, self.out_cap = C, out_cap

    def step(self, dx, n, mid, out):
        _, c, p, _ = self.rf.work_dev(dx.data_ptr(), n, mid.data_ptr(), self.mid_cap)
        for ch, a in enumerate(self.au):
            a.work_dev(mid.data_ptr() + 4 * ch * self.mid_cap, p, out.data_ptr() + 4 * ch * self.out_cap, self.out_cap)
        return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, taps, rf, at, au, n in shapes():
        if a.only and a.only not in name:
            continue
        C = len(taps)
        x = (np.random.default_rng(1).standard_normal(2 * n).astype(np.float32) * 0.5)
        dx = torch.from_numpy(x).cuda()
        out_cap = n * rf[0] * au[0] // (rf[1] * au[1]) + 64
        ya = torch.empty(C * out_cap, dtype=torch.float32, device="cuda")
        yb = torch.empty(C * out_cap, dtype=torch.float32, device="cuda")
        mid = torch.empty(C * (n * rf[0] // rf[1] + 16), dtype=torch.float32, device="cuda")
        times = {"A": [], "B": []}
        pa = pb = 0
        # both ways keep their handles over the steps, as a running graph does: every step is the next window of one stream
        # (the receiver's internal buffer grows during the warm-up steps, the existing blocks' buffers are made above)
        blk = rr.FmReceiver(taps, rf[0], rf[1], at, au[0], au[1], 1.0, rr.ATAN2_EXACT, 0.5)
        ex = Existing(taps, rf, at, au, n, out_cap)
        for it in range(a.warmup + a.steps):
            for k in ("A", "B"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == "A":
                    pa = blk.work_dev(dx.data_ptr(), n, ya.data_ptr(), out_cap)[2]
                else:
                    pb = ex.step(dx, n, mid, yb)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        del blk, ex
        comp_bytes = (8 + C * 4 * rf[0] * au[0] / (rf[1] * au[1])) * n
        row = {"shape": name, "nchan": C, "audio_out_per_channel": pa}
        for k in ("A", "B"):
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["A_beats_B_by_more_than_B_iqr"] = bool(row["B_ms"] - row["A_ms"] > row["B_iqr_ms"])
        row["in_msps_A"] = round(n / row["A_ms"] / 1e3, 1)
        row["compulsory_MB"] = round(comp_bytes / 1e6, 2)
        row["A_of_8TBps"] = round(comp_bytes / (row["A_ms"] * 1e-3) / 8e12, 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
