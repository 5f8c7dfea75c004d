#!/usr/bin/env python3
"""SymbolSync on the device (rr_symbol_sync_create) against what the streaming receivers did without it, same box, interleaved, the
demodulated samples resident in HBM.

    tools/symsync_probe.py [--steps 5] [--warmup 1] [--out profiles/symsync_probe.md]

The samples are random NRZ levels held over sps samples with noise and a clock offset of their own per stream; the parameters are
ax25-9600-rx's (sps 50000 / 9600, max_deviation 0.1, taps [0.0001, 0.99999999]).  Shapes: 1 stream x 1,024,000 samples (the
reference's f32 stream capacity), 32 and 256 streams x 4,000,000 (what one rr_fm_multi step of BASELINE configs[3] delivers per
channel: 24,000,000 samples 1:6), 4096 x 16,384.  Per shape, for both stream-to-lane mappings of the clock kernel
(rr_build_opts.sync_lanes = 1 and 64), in turn:
  (P) one rr_symbol_sync_push_dev of the window with the clock output, synchronised, host-timed
  (1, 2, 3) the three launches of a push on their own (k_sync_signs, k_sync_clock, k_sync_gather), from rr_block_profile of handles
      built with rr_build_opts.sync_prof_launch
and once per shape:
  (H) the path the block replaces: the download of the samples (D), rustradio_amd/csrc/symsync_core.hpp compiled by this probe
      for one host core and run over every stream in turn (S; over a private copy of at most --host-streams streams, scaled to
      all of them), the upload of the symbols (U)
  (Q) rr_quaddemod over as many samples (over at most 1e8 of them, scaled): the yardstick every probe here uses
and a sweep over 1 .. 64 streams of 262,144 samples with the library's own mapping: the stream count from which P beats H.
Reported: the median ms with the interquartile range, and the per-lane rate of the clock kernel (samples of ONE stream per second).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustradio_amd as rr  # noqa: E402

PRM = (50000.0 / 9600.0, 0.1, [0.0001, 0.99999999])

HOST_SRC = r"""
#include "symsync_host.hpp"
extern "C" long symsync_host_run(const float* x, long n, float sps, float dev, const float* taps, long ntaps, float* syms, float* clk) {
    using namespace rr;
    const SyncParams p = symsync_params(sps, dev, taps, (size_t)ntaps);
    SyncState s;
    sync_init(s, p);
    long k = 0;
    for (long i = 0; i < n; i++) {
        float c;
        if (sync_step(s, p, x[i] > 0.0f, &c)) { syms[k] = x[i]; clk[k] = c; k++; }
    }
    return k;
}
"""


def host_core():
    """symsync_core.hpp for one host core, as the reference block runs: sample by sample, straight off the samples"""
    d = tempfile.mkdtemp(prefix="symsync_probe_")
    src, so = os.path.join(d, "host.cpp"), os.path.join(d, "host.so")
    open(src, "w").write(HOST_SRC)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "rustradio_amd", "csrc"),
                    src, "-o", so], check=True)
    L = C.CDLL(so)
    L.symsync_host_run.argtypes = [C.c_void_p, C.c_long, C.c_float, C.c_float, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    L.symsync_host_run.restype = C.c_long
    return L


def signal(ns, n, seed):
    """ns x n on the device: +-1 levels held over sps (1 + offset_c) samples, Gaussian noise of sigma 0.15"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((ns, n), dtype=torch.float32, device="cuda")
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    nsym = int(n / PRM[0] * 1.01) + 2
    for c in range(ns):
        per = PRM[0] * (1.0 + ((c * 5) % 13 - 6) * 0.0005)
        lv = torch.randint(0, 2, (nsym,), generator=g, device="cuda", dtype=torch.int32).to(torch.float32) * 2.0 - 1.0
        x[c] = lv[torch.floor(i / per).to(torch.int64)]
    for c0 in range(0, ns, 64):
        x[c0:c0 + 64] += 0.15 * torch.randn(x[c0:c0 + 64].shape, generator=g, device="cuda", dtype=torch.float32)
    return x


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def time_push(h, x, syms, clk, steps, warmup):
    ns, n = x.shape
    t = []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.push_dev(x.data_ptr(), n, n, syms.data_ptr(), clk.data_ptr(), n)
        torch.cuda.synchronize()
        if it >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


def time_launch(k, lanes, ns, x, syms, clk, steps, warmup):
    """launch k of a push alone, from the events around it"""
    n = x.shape[1]
    with rr.build_options(sync_lanes=lanes, sync_prof_launch=k):
        h = rr.SymbolSync(*PRM, nstreams=ns)
    t = []
    for it in range(warmup + steps):
        h.set_profiling(it >= warmup)
        h.push_dev(x.data_ptr(), n, n, syms.data_ptr(), clk.data_ptr(), n)
        torch.cuda.synchronize()
        if it >= warmup:
            t.append(h.profile()[0])
    return t


def host_path(L, x, counts, steps, warmup, host_streams):
    """D + S + U of one window -> ({D, S, U: times}, symbols of stream 0 on the host)"""
    ns, n = x.shape
    taps = np.asarray(PRM[2], np.float32)
    times = {"D": [], "S": [], "U": []}
    m = min(ns, host_streams)
    hs, hc = np.zeros((m, n), np.float32), np.zeros((m, n), np.float32)
    total = int(counts.sum())
    up = torch.empty(max(total, 1), dtype=torch.float32, device="cuda")
    k0 = 0
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hx = x.cpu()
        t1 = time.perf_counter()
        a = hx.numpy()[:m].copy()           # (S reads a private copy: the first touch of the download's pages is in neither D nor S)
        t1b = time.perf_counter()
        for c in range(m):
            k = L.symsync_host_run(a[c].ctypes.data, n, PRM[0], PRM[1], taps.ctypes.data, len(taps), hs[c].ctypes.data, hc[c].ctypes.data)
            if c == 0:
                k0 = k
        t2 = time.perf_counter()
        pay = torch.from_numpy(np.zeros(max(total, 1), np.float32))         # (as many symbols as the window produced)
        t3 = time.perf_counter()
        up.copy_(pay)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if it >= warmup:
            times["D"].append((t1 - t0) * 1e3)
            times["S"].append((t2 - t1b) * 1e3 * ns / m)
            times["U"].append((t4 - t3) * 1e3)
        del hx
    return times, hs[0, :k0].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-streams", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symsync_probe.md"))
    a = ap.parse_args()
    L = host_core()
    rows = []
    for ns, n in ((1, 1_024_000), (32, 4_000_000), (256, 4_000_000), (4096, 16_384)):
        x = signal(ns, n, 1000 + ns)
        syms, clk = torch.empty_like(x), torch.empty_like(x)
        row = {"streams": ns, "samples_per_stream": n}
        counts = None
        for lanes in (1, 64):
            with rr.build_options(sync_lanes=lanes):
                h = rr.SymbolSync(*PRM, nstreams=ns)
            assert h.streams_per_wave == lanes
            row[f"P{lanes}_ms"], row[f"P{lanes}_iqr_ms"] = med(time_push(h, x, syms, clk, a.steps, a.warmup))
            counts = h.produced().astype(np.int64)
            del h
            for k in (1, 2, 3):
                row[f"L{k}_{lanes}_ms"], row[f"L{k}_{lanes}_iqr_ms"] = med(time_launch(k, lanes, ns, x, syms, clk, a.steps, a.warmup))
            row[f"lane_rate_{lanes}_Msps"] = round(n / (row[f"L2_{lanes}_ms"] * 1e-3) / 1e6, 2)
        row["default_lanes"] = rr.SymbolSync(*PRM, nstreams=ns).streams_per_wave
        # a fresh handle's first window against the host core's: the same symbols
        h = rr.SymbolSync(*PRM, nstreams=ns)
        h.push_dev(x.data_ptr(), n, n, syms.data_ptr(), clk.data_ptr(), n)
        counts = h.produced().astype(np.int64)
        first = syms[0, :int(counts[0])].cpu().numpy()
        del h
        ht, hsyms = host_path(L, x, counts, a.steps, a.warmup, a.host_streams)
        assert np.array_equal(first.view(np.uint32), hsyms.view(np.uint32)), "device and host core disagree"
        for k in ("D", "S", "U"):
            row[k + "_ms"], row[k + "_iqr_ms"] = med(ht[k])
        tot = np.asarray(ht["D"]) + np.asarray(ht["S"]) + np.asarray(ht["U"])
        row["H_ms"], row["H_iqr_ms"] = med(tot)
        row["host_rate_Msps"] = round(ns * n / (row["S_ms"] * 1e-3) / 1e6, 2)
        row["symbols"] = int(counts.sum())
        del syms, clk
        q = rr.QuadratureDemod(1.0)
        N = min(ns * n, 100_000_000)                  # (the sizes the other probes run it at; scaled to the shape's samples)
        qi = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
        qo = torch.empty(N, dtype=torch.float32, device="cuda")
        t = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.work_dev(qi.data_ptr(), N, qo.data_ptr(), N)
            torch.cuda.synchronize()
            if it >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3 * (ns * n) / N)
        row["Q_ms"], row["Q_iqr_ms"] = med(t)
        best = min(row["P1_ms"], row["P64_ms"])
        row["H_over_best_P"] = round(row["H_ms"] / best, 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, qi, qo, q
        torch.cuda.empty_cache()
    # the stream count from which the device wins
    sweep = []
    n = 262_144
    x_all = signal(64, n, 77)
    for ns in (1, 2, 4, 8, 16, 32, 64):
        x = x_all[:ns].contiguous()
        syms, clk = torch.empty_like(x), torch.empty_like(x)
        h = rr.SymbolSync(*PRM, nstreams=ns)
        p = time_push(h, x, syms, clk, a.steps, a.warmup)
        counts = h.produced().astype(np.int64)
        ht, _ = host_path(L, x, counts, a.steps, a.warmup, 64)
        tot = np.asarray(ht["D"]) + np.asarray(ht["S"]) + np.asarray(ht["U"])
        r = {"streams": ns, "samples_per_stream": n, "lanes": h.streams_per_wave}
        r["P_ms"], r["P_iqr_ms"] = med(p)
        r["H_ms"], r["H_iqr_ms"] = med(tot)
        r["device_wins"] = bool(r["H_ms"] - r["P_ms"] >= r["H_iqr_ms"] + r["P_iqr_ms"])
        print(json.dumps(r), flush=True)
        sweep.append(r)
        del h, x, syms, clk
    wins = [r["streams"] for r in sweep if r["device_wins"]]
    first_win = None
    for r in sweep:
        if all(q["device_wins"] for q in sweep if q["streams"] >= r["streams"]):
            first_win = r["streams"]
            break
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_symbol_sync_create: SymbolSync for N streams on the device, the samples resident in HBM\n\n"
                f"`tools/symsync_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; median over the steps (interquartile range in\n"
                "brackets).  P = one rr_symbol_sync_push_dev with the clock output, synchronised and host-timed, with 1 and with 64\n"
                "streams per wave of the clock kernel; signs / clock / gather = its three launches on their own (HIP events around the\n"
                "launch, rr_block_profile); lane rate = samples of ONE stream per second through the clock kernel.  H = the path the\n"
                "block replaces: D, the download of the samples, + S, symsync_core.hpp on one host core over every stream in turn\n"
                f"(measured over a private copy of at most {a.host_streams} streams and scaled), + U, the upload of the symbols.  Q = rr_quaddemod over as many\n"
                "samples (at most 1e8, scaled).  Parameters: ax25-9600-rx's.\n\n"
                "| streams x samples | lanes | P ms | signs ms | clock ms | gather ms | lane rate Msample/s | D ms | S ms | U ms | H ms | host core Msample/s | Q ms | H / best P |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            for lanes in (1, 64):
                mark = " (default)" if r["default_lanes"] == lanes else ""
                f.write(f"| {r['streams']:,} x {r['samples_per_stream']:,} | {lanes}{mark} | {r[f'P{lanes}_ms']} ({r[f'P{lanes}_iqr_ms']}) | "
                        f"{r[f'L1_{lanes}_ms']} ({r[f'L1_{lanes}_iqr_ms']}) | {r[f'L2_{lanes}_ms']} ({r[f'L2_{lanes}_iqr_ms']}) | "
                        f"{r[f'L3_{lanes}_ms']} ({r[f'L3_{lanes}_iqr_ms']}) | {r[f'lane_rate_{lanes}_Msps']} | {r['D_ms']} ({r['D_iqr_ms']}) | "
                        f"{r['S_ms']} ({r['S_iqr_ms']}) | {r['U_ms']} ({r['U_iqr_ms']}) | {r['H_ms']} ({r['H_iqr_ms']}) | {r['host_rate_Msps']} | "
                        f"{r['Q_ms']} ({r['Q_iqr_ms']}) | {r['H_over_best_P']} |\n")
        f.write("\nThe stream count from which the device wins (streams x 262,144 samples, the library's own mapping; the device wins when\n"
                "the medians are apart by at least the sum of the interquartile ranges):\n\n"
                "| streams | lanes | P ms | H ms | device wins |\n|---|---|---|---|---|\n")
        for r in sweep:
            f.write(f"| {r['streams']} | {r['lanes']} | {r['P_ms']} ({r['P_iqr_ms']}) | {r['H_ms']} ({r['H_iqr_ms']}) | {'yes' if r['device_wins'] else 'no'} |\n")
        f.write(f"\nThe device wins from {first_win} streams on (single wins: {wins}).\n" if first_win else
                f"\nThe device wins at no stream count of the sweep without a loss above it (single wins: {wins}).\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows + sweep) + "\n```\n")


if __name__ == "__main__":
    main()
