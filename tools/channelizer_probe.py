#!/usr/bin/env python3
"""Channelizer against FmMulti and the per-channel composition, same box, interleaved A/B, device-resident input.

    tools/channelizer_probe.py [--steps 20] [--warmup 3] [--only ROWKIND]

Per shape three blocks on the same taps and the same device window:
  (a) rr_channelizer (Complex out)        (b) rr_fm_multi (f32 out)
  (c) nchan x (FftFilter, RationalResampler) GPU blocks chained through a device buffer
One step = one work_dev() call of each block over the whole window, in turn (a, b, c, a, b, c, ...), synchronised; the
median over the timed steps is reported with input Msamples/s and the compulsory traffic (8 B in + nchan x 8 B x I / D out per
input sample) / time / 8 TB/s.  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/channelizer_probe.py`.
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


def shapes():
    proto = rr.low_pass_complex(multi.CFG4_FS, 100e3, 12.5e3)
    c32 = multi.cfg4_taps(proto, list(multi.shard_channels(32, 1, 0)))
    rtl = np.asarray(rr.low_pass_complex(250e3, 40e3, 1e3), np.complex64)[None, :]
    return [("configs[3] 32ch 463 taps 1:6", c32, 1, 6, 2_400_000),
            ("rtl_downsampled 1ch 1:5", rtl, 1, 5, 24_000_000),
            ("32ch 463 taps 1:50", c32, 1, 50, 2_400_000)]


class Composition:
    """nchan x (FftFilter, RationalResampler) on device windows: the filter of channel c into a full-rate buffer, the resampler
    from it into channel c's output"""

    def __init__(self, taps, I, D, n):
        self.f = [rr.FftFilter(t) for t in taps]
        self.r = [rr.RationalResampler(I, D) for _ in taps]
        self.mid = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        self.out = torch.empty(2 * (n * I // D + 16), dtype=torch.float32, device="cuda")

    def step(self, dx, n):
        for f, r in zip(self.f, self.r):
            _, c, p, _ = f.work_dev(dx.data_ptr(), n, self.mid.data_ptr(), n)
            r.work_dev(self.mid.data_ptr(), p, self.out.data_ptr(), self.out.numel() // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    rows = []
    for name, taps, I, D, n in shapes():
        if a.only and a.only not in name:
            continue
        C = len(taps)
        x = (np.random.default_rng(1).standard_normal(2 * n).astype(np.float32) * 0.5)
        dx = torch.from_numpy(x).cuda()
        cap = n * I // D + 16
        ych = torch.empty(2 * C * cap, dtype=torch.float32, device="cuda")
        yfm = torch.empty(C * cap, dtype=torch.float32, device="cuda")
        blocks = {}

        def fresh():
            blocks["a"] = rr.Channelizer(taps, I, D)
            blocks["b"] = rr.FmMulti(taps, I, D, 1.0)

        comp = Composition(taps, I, D, n)
        times = {"a": [], "b": [], "c": []}
        for it in range(a.warmup + a.steps):
            fresh()                                   # every step starts a stream: the whole window is one call's work
            for k in ("a", "b", "c"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == "a":
                    blocks["a"].work_dev(dx.data_ptr(), n, ych.data_ptr(), cap)
                elif k == "b":
                    blocks["b"].work_dev(dx.data_ptr(), n, yfm.data_ptr(), cap)
                else:
                    comp.step(dx, n)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
            if it < a.warmup:
                comp = Composition(taps, I, D, n)
        for k, label in (("a", "channelizer"), ("b", "fm_multi"), ("c", "composition")):
            ms = float(np.median(times[k]))
            out_b = C * (8 if k != "b" else 4) * I / D
            comp_bytes = (8 + out_b) * n
            rows.append({"shape": name, "block": label, "nchan": C, "ms_per_step": round(ms, 4),
                         "in_msps": round(n / ms / 1e3, 1), "compulsory_MB": round(comp_bytes / 1e6, 2),
                         "of_8TBps": round(comp_bytes / (ms * 1e-3) / 8e12, 4)})
            print(json.dumps(rows[-1]), flush=True)
        ra = next(r for r in rows if r["shape"] == name and r["block"] == "channelizer")
        rc = next(r for r in rows if r["shape"] == name and r["block"] == "composition")
        print(json.dumps({"shape": name, "composition_over_channelizer": round(rc["ms_per_step"] / ra["ms_per_step"], 2)}), flush=True)
        del blocks, comp


if __name__ == "__main__":
    main()
