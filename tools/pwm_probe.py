#!/usr/bin/env python3
"""The PWM decoder on the device (rr_pwm_decoder_create, Complex input) against the path it replaces, same box, interleaved, the
Complex samples resident in HBM.

    tools/pwm_probe.py [--steps 10] [--warmup 2] [--out profiles/pwm_probe.md]

Settings of examples/restaurant_pager.rs at 125 kS/s: short 26, long 80, frame gap 110, reset gap 914, 25 bits, min_repeats 3,
Delimiter.  Shapes: 2^22 samples of noise with a transmission (five repeats of a 25-bit word) every 125,000 samples; the first
16,384 of them as a small push; and 2^20 samples with an edge on every sample (power 1, 0, 1, 0, ...), where every pulse is one
item of the decoder's one-wave walk.  Per shape, in turn (P, F, M, D, Q, P, ...):
  (P) one rr_pwm_decoder_push_dev of the Complex samples, synchronised
  (F) rr_pwm_frames and rr_pwm_frame_bits behind it: the counts, the records and the bits come down and are checked
  (M) rr_complex_to_mag2 over the same samples: the first step of the path the block replaces
  (D) the download of the power stream to the host, 4 B per sample
  (Q) rr_quaddemod over as many Complex samples: the project's usual yardstick
and once per shape (H) the sequential machine of pwm_host.hpp over the downloaded power stream on one host core
(tools/pwm_host_machine.cpp, g++ -O2), which also has to give the device's frame count.
Reported: the median ms with the interquartile range, kernel launches per push, the frames of a push, and whether P + F is
slower than M + D + H: it is when the medians are apart by at least the sum of the interquartile ranges."""
from __future__ import annotations

import argparse
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

PAGER = dict(short=26, long=80, tol=27, fgap=110, rgap=914, bits=25, min_repeats=3)


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def pager_stream(rng, n):
    env = np.zeros(n, np.float32)
    for t0 in range(20_000, n - 20_000, 125_000):
        at = t0
        word = rng.integers(0, 2, PAGER["bits"])
        for _ in range(5):
            for b in word:
                w = PAGER["short"] if b else PAGER["long"]
                env[at:at + w] = 1.0
                at += PAGER["short"] + PAGER["long"]
            env[at:at + PAGER["short"]] = 1.0
            at += PAGER["short"] + 300
    return (env + rng.normal(0, 0.05, n) + 1j * rng.normal(0, 0.05, n)).astype(np.complex64)


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pwm_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "pwm_host_machine")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "pwm_host_machine.cpp"), "-o", exe], check=True)
    big = pager_stream(rng, 1 << 22)
    shapes = (("pager, 2^22 samples, a transmission every 125,000", big), ("pager, the first 16,384 samples", big[:16384]),
              ("an edge on every sample, 2^20 samples", np.resize(np.array([1.0, 0.0], np.complex64), 1 << 20)))
    rows = []
    for name, z in shapes:
        n = len(z)
        dz = torch.from_numpy(z.view(np.float32).copy()).cuda()
        power = torch.empty(n, dtype=torch.float32, device="cuda")
        mag, quad = rr.ComplexToMag2(), rr.QuadratureDemod(1.0)
        times = {"P": [], "F": [], "M": [], "D": [], "Q": []}
        nl, frames = 0, 0
        for it in range(a.warmup + a.steps):
            # (a fresh handle per step: every push sees the same stream from its start)
            d = rr.PwmDecoder(0.5, PAGER["short"], PAGER["long"], PAGER["fgap"], PAGER["rgap"], frame_bits=PAGER["bits"],
                              min_repeats=PAGER["min_repeats"], delimiter=True, dtype=np.complex64)
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                if k == "P":
                    d.push_dev(dz.data_ptr(), n)
                elif k == "F":
                    frames = len(d.frames())
                    d.frame_bits()
                elif k == "M":
                    assert mag.work_dev(dz.data_ptr(), n, power.data_ptr(), n)[2] == n
                elif k == "D":
                    host_power = power.cpu().numpy()
                else:
                    quad.work_dev(dz.data_ptr(), n, power.data_ptr(), n)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                if k == "P":
                    nl = launches() - l0
            del d
        pfile = os.path.join(tmp, "power.f32")
        host_power.tofile(pfile)
        res = subprocess.run([exe, pfile, *[str(PAGER[k]) for k in ("short", "long", "tol", "fgap", "rgap", "bits", "min_repeats")], "1",
                              str(a.steps)], capture_output=True, text=True, check=True)
        host = [ln.split() for ln in res.stdout.strip().splitlines()]
        assert all(int(h[0]) == frames for h in host), (name, frames, host[:2])
        row = {"shape": name, "samples": int(n), "frames_per_push": int(frames), "P_launches": nl}
        for k in times:
            row[k + "_ms"], row[k + "_iqr_ms"] = med(times[k])
        row["H_ms"], row["H_iqr_ms"] = med([float(h[1]) for h in host])
        row["PF_ms"], row["PF_iqr_ms"] = med(np.asarray(times["P"]) + np.asarray(times["F"]))
        old = np.asarray(times["M"]) + np.asarray(times["D"]) + np.asarray([float(h[1]) for h in host])
        row["MDH_ms"], row["MDH_iqr_ms"] = med(old)
        row["P_Msample_per_s"] = round(n / (row["P_ms"] * 1e-3) / 1e6, 1)
        row["MDH_over_PF"] = round(row["MDH_ms"] / row["PF_ms"], 2)
        row["Q_over_P"] = round(row["Q_ms"] / row["P_ms"], 3)
        row["PF_slower_than_MDH"] = bool(row["PF_ms"] - row["MDH_ms"] >= row["PF_iqr_ms"] + row["MDH_iqr_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_pwm_decoder_create: [ComplexToMag2 ->] PwmDecoder on the device, the Complex samples resident in HBM\n\n"
                f"`tools/pwm_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed calls, synchronised, median over the\n"
                "steps (interquartile range in brackets).  restaurant_pager settings at 125 kS/s.  P = one rr_pwm_decoder_push_dev of the\n"
                "Complex samples, F = rr_pwm_frames + rr_pwm_frame_bits behind it; the path they replace: M = rr_complex_to_mag2, D = the\n"
                "download of the power stream, H = pwm_host.hpp's sequential machine on one host core; Q = rr_quaddemod over as many\n"
                "Complex samples (the usual yardstick).  P + F counts as slower than M + D + H when the medians are apart by at least the\n"
                "sum of the interquartile ranges.\n\n"
                "| shape | samples | frames per push | P ms | launches | P Msample/s | F ms | P + F ms | M ms | D ms | H ms | M + D + H ms | Q ms | (M + D + H) / (P + F) | Q / P | P + F slower |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['samples']:,} | {r['frames_per_push']:,} | {r['P_ms']} ({r['P_iqr_ms']}) | {r['P_launches']} | "
                    f"{r['P_Msample_per_s']} | {r['F_ms']} ({r['F_iqr_ms']}) | {r['PF_ms']} ({r['PF_iqr_ms']}) | {r['M_ms']} ({r['M_iqr_ms']}) | "
                    f"{r['D_ms']} ({r['D_iqr_ms']}) | {r['H_ms']} ({r['H_iqr_ms']}) | {r['MDH_ms']} ({r['MDH_iqr_ms']}) | {r['Q_ms']} ({r['Q_iqr_ms']}) | "
                    f"{r['MDH_over_PF']} | {r['Q_over_P']} | {'yes' if r['PF_slower_than_MDH'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
