#!/usr/bin/env python3
"""The N-stream AFSK tone demodulator (rr_afsk_demod_create) against the path it replaces and against its consumer, same box,
interleaved, the audio resident in HBM.

    tools/afsk_probe.py [--steps 5] [--warmup 1] [--b-streams 4] [--out profiles/afsk_probe.md]

The audio is Bell 202 AFSK made on the device: random levels held over fs / 1200 samples, 2200 Hz for a positive level and 1200 Hz
otherwise, phase-continuous, 0.5 cos + 0.02 N(0, 1).  Two settings: fs 12,000 with low_pass(12000, 1100, 100) (289 taps, 10 samples
per symbol) and fs 50,000 with low_pass(50000, 1100, 100) (1,205 taps, 41.67 samples per symbol: examples/ax25-1200-rx.rs); Hilbert
65 taps, offset -1700 * 2 pi / fs.  Shapes: 32 x 480,000, 256 x 480,000, 4,096 x 16,384 and 1 x 1,000,000, each at both settings.
Per shape, in turn, every step a further window of the same streams (steady state):
  (A) one rr_afsk_demod_push_dev, synchronised and host-timed; and the kernel alone from the events around it (rr_block_profile)
  (B) the path it replaces, per stream rr_hilbert -> rr_quaddemod -> rr_fftfilter_float -> rr_add_const through rr_block_work_dev
      until each block has taken its window, synchronised once at the end and host-timed; measured over at most --b-streams streams
      and scaled to all of them (the streams are independent handles run one after the other)
  (C) the consumer: one rr_symbol_sync_push_dev over A's output
Reported: launches (rr_debug_kernel_launches), median ms with the interquartile range, the rate of the low-pass's multiply-adds in
A's kernel (2 nstreams n L / kernel time; the Hilbert sums and the halo are not counted), and, over the first 100,000 outputs of
stream 0 from fresh handles, how much of the tests' bound against the float64 definition A and B use (both <= 1: A equals B within
the bound).
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

HIL, TOL, CHECK = 65, 1e-5, 100_000
SETTINGS = {289: 12000.0, 1205: 50000.0}


def signal(ns, n, fs, seed):
    """ns x n float32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sps = fs / 1200.0
    x = torch.empty((ns, n), dtype=torch.float32, device="cuda")
    idx = torch.floor(torch.arange(n, device="cuda", dtype=torch.float64) / sps).to(torch.int64)
    nsym = int(idx[-1].item()) + 1
    for c0 in range(0, ns, 32):
        m = min(32, ns - c0)
        lv = torch.randint(0, 2, (m, nsym), generator=g, device="cuda", dtype=torch.int32)
        f = torch.where(lv[:, idx] > 0, 2200.0, 1200.0).to(torch.float64)
        ph = 2.0 * np.pi * torch.cumsum(f, dim=1) / fs
        x[c0:c0 + m] = (0.5 * torch.cos(ph)).to(torch.float32) + 0.02 * torch.randn((m, n), generator=g, device="cuda", dtype=torch.float32)
        del lv, f, ph
    return x


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


class Unfused:
    """one stream of the path the block replaces.  The window between two blocks is the probe's: a block writes behind what the
    next one left last time, and what a block leaves (the history a filter keeps, the sample QuadratureDemod holds back,
    FftFilterFloat's partial block) is moved to the front of its window — one small device copy per block and step, inside B's time,
    where a graph's rings would wrap instead."""
    SLACK = 65536

    def __init__(self, taps, offset, n):
        self.blocks = [rr.Hilbert(HIL), rr.QuadratureDemod(1.0), rr.FftFilterFloat(taps), rr.AddConst(offset)]
        self.cap = n + self.SLACK
        self.fl = [b.in_dtype.itemsize // 4 for b in self.blocks]                       # floats per input element
        self.buf = [torch.empty(self.cap * k, dtype=torch.float32, device="cuda") for k in self.fl]
        self.left = [0, 0, 0, 0]

    def step(self, row, n, d_out, out_cap):
        """the next n samples of the stream (a device tensor) -> outputs written at d_out"""
        self.buf[0][self.left[0]:self.left[0] + n] = row[:n]
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


def f64_bound(x, hil, taps, offset):
    """the float64 definition over the host row x and the tests' per-output bound (tests/afsk_model.py)"""
    x, hil, taps = np.asarray(x, np.float64), np.asarray(hil, np.float64), np.asarray(taps, np.float64)
    H, T = len(hil), len(x)
    xp = np.concatenate([np.zeros(H), x])
    a = xp[H // 2:H // 2 + T] + 1j * np.convolve(xp, hil)[H - 1:H - 1 + T]
    d = np.angle(a[1:] * np.conj(a[:-1]))
    y = np.convolve(d, taps)[:len(d)]
    mag = np.abs(a)
    eps = TOL * float(mag.max())
    b = TOL * np.pi + eps / np.maximum(mag[:-1], 1e-30) + eps / np.maximum(mag[1:], 1e-30)
    return y + offset, np.convolve(b, np.abs(taps))[:len(b)] + TOL * float(np.max(np.abs(y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--b-streams", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afsk_probe.md"))
    a = ap.parse_args()
    hil = rr.hilbert_taps(rr.make_window(rr.WIN_HAMMING, HIL))
    rows = []
    for L, fs in SETTINGS.items():
        taps = rr.low_pass(fs, 1100.0, 100.0)
        assert len(taps) == L
        offset = -1700.0 * 2.0 * np.pi / fs
        sync_prm = (fs / 1200.0, 0.5, [0.1, 0.9])
        for ns, n in ((32, 480_000), (256, 480_000), (4096, 16_384), (1, 1_000_000)):
            x = signal(ns, n, fs, 100 * L + ns)
            soft, syms = torch.empty_like(x), torch.empty_like(x)
            row = {"streams": ns, "samples_per_stream": n, "ntaps": L, "fs": fs}
            # first window of fresh handles: A and B against float64 on stream 0
            m = min(n, CHECK + 1)
            want, bound = f64_bound(x[0, :m].cpu().numpy(), hil, taps, offset)
            h = rr.AfskDemod(ns, HIL, taps, 1.0, offset)
            p = h.push_dev(x.data_ptr(), n, n, soft.data_ptr(), n)
            torch.cuda.synchronize()
            assert p == n - 1
            got_a = soft[0, :m - 1].cpu().numpy().astype(np.float64)
            row["used_A"] = round(float(np.max(np.abs(got_a - want) / bound)), 4)
            mb = min(ns, a.b_streams)
            un = [Unfused(taps, offset, n) for _ in range(mb)]
            outs = torch.empty((mb, n + 8), dtype=torch.float32, device="cuda")
            pb = un[0].step(x[0], n, outs[0].data_ptr(), n + 8)
            torch.cuda.synchronize()
            kb = min(pb, m - 1)
            got_b = outs[0, :kb].cpu().numpy().astype(np.float64)
            row["B_first_outputs"] = pb
            row["used_B"] = round(float(np.max(np.abs(got_b - want[:kb]) / bound[:kb])), 4) if kb else None
            row["A_equals_B_within_bound"] = bool(kb and row["used_A"] <= 1.0 and row["used_B"] <= 1.0)
            for c in range(1, mb):
                un[c].step(x[c], n, outs[c].data_ptr(), n + 8)
            ss = rr.SymbolSync(*sync_prm, nstreams=ns)
            tA, tK, tB, tC = [], [], [], []
            for it in range(a.warmup + a.steps):
                x = signal(ns, n, fs, 100 * L + ns + 7 * (it + 1)) if ns * n <= 16_000_000 else x     # (a further window)
                timed = it >= a.warmup
                torch.cuda.synchronize()
                h.set_profiling(True)
                l0 = launches()
                t0 = time.perf_counter()
                p = h.push_dev(x.data_ptr(), n, n, soft.data_ptr(), n)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                row["A_launches"] = launches() - l0
                kms = h.profile()[0]
                assert p == n
                l0 = launches()
                t2 = time.perf_counter()
                for c in range(mb):
                    un[c].step(x[c], n, outs[c].data_ptr(), n + 8)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                row["B_launches"] = round((launches() - l0) * ns / mb)
                l0 = launches()
                t4 = time.perf_counter()
                ss.push_dev(soft.data_ptr(), n, p, syms.data_ptr(), None, n)
                torch.cuda.synchronize()
                t5 = time.perf_counter()
                row["C_launches"] = launches() - l0
                if timed:
                    tA.append((t1 - t0) * 1e3)
                    tK.append(kms)
                    tB.append((t3 - t2) * 1e3 * ns / mb)
                    tC.append((t5 - t4) * 1e3)
            row["A_ms"], row["A_iqr_ms"] = med(tA)
            row["A_kernel_ms"], row["A_kernel_iqr_ms"] = med(tK)
            row["B_ms"], row["B_iqr_ms"] = med(tB)
            row["C_ms"], row["C_iqr_ms"] = med(tC)
            row["B_streams_measured"] = mb
            row["lowpass_TFLOPs"] = round(2.0 * ns * n * L / (row["A_kernel_ms"] * 1e-3) / 1e12, 2)
            row["per_stream_Msps"] = round(n / (row["A_ms"] * 1e-3) / 1e6, 2)
            row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
            row["C_over_A"] = round(row["C_ms"] / row["A_ms"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del h, un, outs, ss, x, soft, syms
            torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_afsk_demod_create: Hilbert -> QuadratureDemod -> FftFilterFloat -> AddConst for N streams, the audio resident in HBM\n\n"
                f"`tools/afsk_probe.py --steps {a.steps} --warmup {a.warmup} --b-streams {a.b_streams}` on {dev}; median over the steps\n"
                "(interquartile range in brackets), every step a further window of the same streams.  A = one rr_afsk_demod_push_dev,\n"
                "synchronised and host-timed (kernel = the launch alone, HIP events).  B = the path it replaces, per stream rr_hilbert ->\n"
                "rr_quaddemod -> rr_fftfilter_float -> rr_add_const through rr_block_work_dev, one stream after the other, measured over\n"
                f"at most {a.b_streams} streams and scaled.  C = the consumer, one rr_symbol_sync_push_dev over A's output.  used = the share of\n"
                "the tests' bound against the float64 definition over the first 100,000 outputs of stream 0 from fresh handles.  A loss of\n"
                "A (B below A, or C below A: the demodulator is then the chain's bottleneck) is in bold.\n\n"
                "| streams x samples | taps | A launches | A ms | A kernel ms | low-pass TFLOP/s | B launches | B ms | C launches | C ms | B / A | C / A | used A | used B | A = B within the bound |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            ba = f"{r['B_over_A']}" if r["B_over_A"] >= 1 else f"**{r['B_over_A']}**"
            ca = f"{r['C_over_A']}" if r["C_over_A"] >= 1 else f"**{r['C_over_A']}**"
            f.write(f"| {r['streams']:,} x {r['samples_per_stream']:,} | {r['ntaps']:,} | {r['A_launches']} | {r['A_ms']} ({r['A_iqr_ms']}) | "
                    f"{r['A_kernel_ms']} ({r['A_kernel_iqr_ms']}) | {r['lowpass_TFLOPs']} | {r['B_launches']:,} | {r['B_ms']} ({r['B_iqr_ms']}) | "
                    f"{r['C_launches']} | {r['C_ms']} ({r['C_iqr_ms']}) | {ba} | {ca} | {r['used_A']} | {r['used_B']} | "
                    f"{'yes' if r['A_equals_B_within_bound'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
