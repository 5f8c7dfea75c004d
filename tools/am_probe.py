#!/usr/bin/env python3
"""The N-stream AM audio stage (rr_am_demod_create) against a stand-in for the path it replaces and against the library's usual
yardstick, same box, interleaved, the samples resident in HBM.

    tools/am_probe.py [--steps 5] [--warmup 1] [--b-streams 2] [--out profiles/am_probe.md]

The samples are AM made on the device: a carrier of unit amplitude with the envelope 1 + 0.5 cos(w k), plus 1e-3 N(0, 1) per
component.  Shapes (streams x samples per step, taps, ratio):
  1 x 2,500,000, low_pass(2.5e6, 48000, 500) (12,045 taps), 12:625        examples/airspy_am_decode.rs, one second per step
  32 x 2,500,000, the same
  256 x 480,000, low_pass(12000, 1100, 100) (289 taps), 1:1               a short filter, nothing thrown away
  4,096 x 16,384, the same
Per shape, in turn, every step a further window of the same streams (steady state):
  (A) one rr_am_demod_push_dev, synchronised and host-timed; and the kernel alone from the events around it (rr_block_profile)
  (B) a STAND-IN for the path A replaces.  No block of the library computes |v|, so no path of existing blocks produces A's
      values; per stream rr_complex_to_mag2 -> rr_fftfilter_float -> rr_resampler -> rr_multiply_const through rr_block_work_dev
      moves the same traffic and does the same arithmetic but for the square root.  Synchronised once at the end and host-timed;
      measured over at most --b-streams streams and scaled to all of them (independent handles, one after the other)
  (Q) the yardstick of the other probe files: one rr_quaddemod over as many Complex samples (streams x samples, one window)
Reported: launches (rr_debug_kernel_launches), median ms with the interquartile range, the rate of A's multiply-adds (2 x outputs
x taps / kernel time), and, over the first outputs of stream 0 from a fresh handle, how much of the tests' bound against the
float64 definition A uses.
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

CHECK = 400                                    # outputs of stream 0 held against float64


def signal(ns, n, seed):
    """ns x n Complex on the device, as float32 (ns, 2 n)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((ns, 2 * n), dtype=torch.float32, device="cuda")
    k = torch.arange(n, device="cuda", dtype=torch.float64)
    for c0 in range(0, ns, 32):
        m = min(32, ns - c0)
        wa = 0.002 + 0.0001 * torch.arange(c0, c0 + m, device="cuda", dtype=torch.float64)[:, None]
        env = 1.0 + 0.5 * torch.cos(wa * k[None, :])
        ph = 0.013 * k[None, :] + 0.1 * c0
        v = x[c0:c0 + m].view(m, n, 2)
        v[:, :, 0] = (env * torch.cos(ph)).to(torch.float32)
        v[:, :, 1] = (env * torch.sin(ph)).to(torch.float32)
        v += 1e-3 * torch.randn((m, n, 2), generator=g, device="cuda", dtype=torch.float32)
        del env, ph
    return x


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


class StandIn:
    """one stream of ComplexToMag2 -> FftFilterFloat -> RationalResampler -> MultiplyConst.  The window between two blocks is the
    probe's: a block writes behind what the next one left last time, and what a block leaves (the filter's partial block) is moved
    to the front of its window — one small device copy per block and step, inside B's time, where a graph's rings would wrap."""
    SLACK = 65536

    def __init__(self, taps, interp, deci, scale, n):
        self.blocks = [rr.ComplexToMag2(), rr.FftFilterFloat(taps), rr.RationalResampler(interp, deci, np.float32), rr.MultiplyConst(scale)]
        self.cap = n + self.SLACK
        self.fl = [b.in_dtype.itemsize // 4 for b in self.blocks]
        self.buf = [torch.empty(self.cap * k, dtype=torch.float32, device="cuda") for k in self.fl]
        self.left = [0] * len(self.blocks)

    def step(self, row, n, d_out, out_cap):
        self.buf[0][2 * self.left[0]:2 * (self.left[0] + n)] = row[:2 * n]
        new = n
        for i, blk in enumerate(self.blocks):
            have, took, out = self.left[i] + new, 0, 0
            last = i == len(self.blocks) - 1
            dst = d_out if last else self.buf[i + 1].data_ptr() + 4 * self.fl[i + 1] * self.left[i + 1]
            room = out_cap if last else self.cap - self.left[i + 1]
            oes = blk.out_dtype.itemsize
            while True:
                st, c, p, need = blk.work_dev(self.buf[i].data_ptr() + 4 * self.fl[i] * took, have - took, dst + oes * out, room - out)
                took += c
                out += p
                if c == 0 and p == 0:
                    break
            rest = have - took
            if rest and took:
                k = self.fl[i]
                self.buf[i][:k * rest] = self.buf[i][k * took:k * have].clone()
            self.left[i] = rest
            new = out
        return new


def f64_used(x, taps, interp, deci, scale, got):
    """the share of the tests' bound (tests/am_model.py) the first len(got) outputs of one stream use"""
    z = x[0::2].astype(np.float64) ** 2 + x[1::2].astype(np.float64) ** 2
    m = np.sqrt(z)
    t = np.asarray(taps, np.float64)
    p = (np.arange(len(got), dtype=np.int64) * deci) // interp
    y = np.convolve(m, t)[:len(m)][p] * scale
    ab = np.convolve(m, np.abs(t))[:len(m)][p]
    b = 1.01 * (len(t) + 2) * 2.0 ** -24 * abs(scale) * ab
    return round(float(np.max(np.abs(got.astype(np.float64) - y) / b)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--b-streams", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "am_probe.md"))
    a = ap.parse_args()
    long_taps, short_taps = rr.low_pass(2.5e6, 48000.0, 500.0), rr.low_pass(12000.0, 1100.0, 100.0)
    assert len(long_taps) == 12045 and len(short_taps) == 289
    shapes = ((1, 2_500_000, long_taps, 12, 625), (32, 2_500_000, long_taps, 12, 625), (256, 480_000, short_taps, 1, 1),
              (4096, 16_384, short_taps, 1, 1))
    scale, rows = 0.5, []
    for ns, n, taps, I, D in shapes:
        L = len(taps)
        x = signal(ns, n, 100 * ns + L)
        h = rr.AmDemod(ns, taps, I, D, scale)
        cap = h.count(n) + 8
        audio = torch.empty((ns, cap), dtype=torch.float32, device="cuda")
        row = {"streams": ns, "samples_per_stream": n, "ntaps": L, "ratio": f"{I}:{D}", "tile_outputs": h.dims()[0]}
        k = h.push_dev(x.data_ptr(), n, n, audio.data_ptr(), cap)
        torch.cuda.synchronize()
        kc = min(k, CHECK)
        need = (kc * D) // I + 1
        row["used_A"] = f64_used(x[0, :2 * need].cpu().numpy(), taps, I, D, scale, audio[0, :kc].cpu().numpy())
        mb = min(ns, a.b_streams)
        un = [StandIn(taps, I, D, scale, n) for _ in range(mb)]
        outs = torch.empty((mb, cap + 8), dtype=torch.float32, device="cuda")
        for c in range(mb):
            un[c].step(x[c], n, outs[c].data_ptr(), cap + 8)
        qd = rr.QuadratureDemod(1.0)
        qout = torch.empty(ns * n, dtype=torch.float32, device="cuda")
        tA, tK, tB, tQ = [], [], [], []
        for it in range(a.warmup + a.steps):
            x = signal(ns, n, 100 * ns + L + 7 * (it + 1)) if ns * n <= 16_000_000 else x      # (a further window)
            timed = it >= a.warmup
            torch.cuda.synchronize()
            h.set_profiling(True)
            l0 = launches()
            t0 = time.perf_counter()
            k = h.push_dev(x.data_ptr(), n, n, audio.data_ptr(), cap)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            row["A_launches"] = launches() - l0
            kms = h.profile()[0]
            l0 = launches()
            t2 = time.perf_counter()
            for c in range(mb):
                un[c].step(x[c], n, outs[c].data_ptr(), cap + 8)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            row["B_launches"] = round((launches() - l0) * ns / mb)
            l0 = launches()
            t4 = time.perf_counter()
            qd.work_dev(x.data_ptr(), ns * n, qout.data_ptr(), ns * n)
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            row["Q_launches"] = launches() - l0
            if timed:
                tA.append((t1 - t0) * 1e3)
                tK.append(kms)
                tB.append((t3 - t2) * 1e3 * ns / mb)
                tQ.append((t5 - t4) * 1e3)
        row["outputs_per_stream"] = k
        row["A_ms"], row["A_iqr_ms"] = med(tA)
        row["A_kernel_ms"], row["A_kernel_iqr_ms"] = med(tK)
        row["B_ms"], row["B_iqr_ms"] = med(tB)
        row["Q_ms"], row["Q_iqr_ms"] = med(tQ)
        row["B_streams_measured"] = mb
        row["sum_TFLOPs"] = round(2.0 * ns * k * L / (row["A_kernel_ms"] * 1e-3) / 1e12, 3)
        row["per_stream_Msps"] = round(n / (row["A_ms"] * 1e-3) / 1e6, 2)
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["Q_over_A"] = round(row["Q_ms"] / row["A_ms"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del h, un, outs, qd, qout, x, audio
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_am_demod_create: norm -> FftFilterFloat -> RationalResampler -> MultiplyConst for N streams, the samples resident in HBM\n\n"
                f"`tools/am_probe.py --steps {a.steps} --warmup {a.warmup} --b-streams {a.b_streams}` on {dev}; one run, median over the steps\n"
                "(interquartile range in brackets), every step a further window of the same streams.  A = one rr_am_demod_push_dev,\n"
                "synchronised and host-timed (kernel = the launch alone, HIP events).  B is a STAND-IN, not the same values: no block of\n"
                "the library computes |v|, so per stream rr_complex_to_mag2 -> rr_fftfilter_float -> rr_resampler -> rr_multiply_const\n"
                f"through rr_block_work_dev, one stream after the other, measured over at most {a.b_streams} streams and scaled: the same traffic\n"
                "and arithmetic but for the square root.  Q = the yardstick, one rr_quaddemod over as many Complex samples.  used = the share\n"
                f"of the tests' bound against the float64 definition over the first {CHECK} outputs of stream 0 from a fresh handle.  A loss\n"
                "of A (B below A) is in bold.\n\n"
                "| streams x samples | taps | ratio | tile | A launches | A ms | A kernel ms | sum TFLOP/s | B launches | B ms | Q ms | B / A | Q / A | used A |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            ba = f"{r['B_over_A']}" if r["B_over_A"] >= 1 else f"**{r['B_over_A']}**"
            f.write(f"| {r['streams']:,} x {r['samples_per_stream']:,} | {r['ntaps']:,} | {r['ratio']} | {r['tile_outputs']} | {r['A_launches']} | "
                    f"{r['A_ms']} ({r['A_iqr_ms']}) | {r['A_kernel_ms']} ({r['A_kernel_iqr_ms']}) | {r['sum_TFLOPs']} | {r['B_launches']:,} | "
                    f"{r['B_ms']} ({r['B_iqr_ms']}) | {r['Q_ms']} ({r['Q_iqr_ms']}) | {ba} | {r['Q_over_A']} | {r['used_A']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
