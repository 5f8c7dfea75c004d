#!/usr/bin/env python3
"""The HDLC deframer on the device (rr_hdlc_deframer_create) against what the receive chain did without it, same box, interleaved,
the bits resident in HBM.

    tools/hdlc_probe.py [--steps 10] [--warmup 2] [--out profiles/hdlc_probe.md]

The bits are what the packet receivers hand to HdlcDeframer: packets through rr_hdlc_framer(FCS | G3RUH | NRZI | SYMBOLS) and back
through rr_bit_decoder(NRZI | DESCRAMBLE), all on the device.  Shapes: 100,000 and 64 packets of 256 random bytes (the framer
probe's), one push of 2^24 random bits, and one all-0xff frame of 65,534 bytes with its checksum, the longest a handle delivers
(max_size 65535 drops a frame of exactly that).  Per shape, in turn (P, F, D, C, P, ...):
  (P) one rr_hdlc_deframer_push_dev of the bits, synchronised
  (F) rr_hdlc_frames behind it: the count, the records and the counters come down and are checked
  (D) the download of the same bits to the host (one byte per bit): what the chain paid before a host deframer could start.
      The host deframer's own time is not in D, so P + F cannot be expected to beat today's path by less than D.
  (C) rr_bit_decoder over as many f32 symbols: the packet-side yardstick (one pass at 5 B per element)
Reported: the median ms with the interquartile range, kernel launches per push, the frames of a push, and whether P + F is
slower than D: it is when the medians are apart by at least the sum of the interquartile ranges.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdlc_model as hm  # noqa: E402
import rustradio_amd as rr  # noqa: E402


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def looped_back(data, P, L):
    """P packets of L bytes -> (the receive side's bits on the device, their f32 symbols)"""
    lens = np.full(P, L, np.uintp)
    starts = (np.arange(P) * L).astype(np.uintp)
    fr = rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0)
    cap = fr.bound(lens)
    d_in = torch.from_numpy(data).cuda()
    sym = torch.empty(cap, dtype=torch.float32, device="cuda")
    fr.push_dev(d_in.data_ptr(), len(data), starts, lens, sym.data_ptr(), cap)
    n = fr.records()[1]
    bits = torch.empty(n, dtype=torch.uint8, device="cuda")
    dec = rr.BitDecoder(nrzi=True, descrambler=(0x21, 0, 16))
    assert dec.work_dev(sym.data_ptr(), n, bits.data_ptr(), n)[2] == n
    torch.cuda.synchronize()
    return bits, sym[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdlc_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    big = 65534 - 2
    shapes = (("100,000 packets of 256 bytes", lambda: looped_back(rng.integers(0, 256, 100_000 * 256, dtype=np.uint8), 100_000, 256), (0, 4096, 0), 100_000),
              ("64 packets of 256 bytes", lambda: looped_back(rng.integers(0, 256, 64 * 256, dtype=np.uint8), 64, 256), (0, 4096, 0), 64),
              ("2^24 random bits", lambda: (torch.from_numpy(rng.integers(0, 2, 1 << 24, dtype=np.uint8)).cuda(), None), (0, 4096, 0), None),
              ("one all-0xff frame of 65,534 bytes", lambda: (torch.from_numpy(np.array(hm.frame_bits(b"\xff" * big), np.uint8)).cuda(), None),
               (0, 65535, rr.HDLC_FIX_BITS), 1))
    rows = []
    for name, make, cfg, want in shapes:
        bits, sym = make()
        n = len(bits)
        if sym is None:
            sym = torch.where(bits != 0, 1.0, -1.0).to(torch.float32)
        d = rr.HdlcDeframer(*cfg)
        dec = rr.BitDecoder(nrzi=True, descrambler=(0x21, 0, 16))
        scratch = torch.empty(n, dtype=torch.uint8, device="cuda")
        times = {"P": [], "F": [], "D": [], "C": []}
        nl, frames = 0, 0
        for it in range(a.warmup + a.steps):
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                if k == "P":
                    d.push_dev(bits.data_ptr(), n)
                elif k == "F":
                    frames = len(d.frames())
                elif k == "D":
                    bits.cpu()
                else:
                    dec.work_dev(sym.data_ptr(), n, scratch.data_ptr(), n)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                if k == "P":
                    nl = launches() - l0
            assert want is None or want <= frames <= want + 1, (name, frames, want)      # (+ 1: the 16 zeros between two pushes of the same bits are an empty frame with a good CRC)
        row = {"shape": name, "bits": int(n), "frames_per_push": int(frames), "stats": list(d.stats()), "P_launches": nl}
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
        pf = np.asarray(times["P"]) + np.asarray(times["F"])
        row["PF_ms"] = round(float(np.median(pf)), 4)
        row["PF_iqr_ms"] = round(float(np.percentile(pf, 75) - np.percentile(pf, 25)), 4)
        row["P_Gbit_per_s"] = round(n / (row["P_ms"] * 1e-3) / 1e9, 2)
        row["D_over_PF"] = round(row["D_ms"] / row["PF_ms"], 2)
        row["C_over_P"] = round(row["C_ms"] / row["P_ms"], 2)
        row["PF_slower_than_D"] = bool(row["PF_ms"] - row["D_ms"] >= row["PF_iqr_ms"] + row["D_iqr_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del d, dec, bits, sym, scratch
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_hdlc_deframer_create: HdlcDeframer on the device, the bits resident in HBM\n\n"
                f"`tools/hdlc_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed calls, synchronised, median over the\n"
                "steps (interquartile range in brackets).  P = one rr_hdlc_deframer_push_dev, F = rr_hdlc_frames behind it, D = the\n"
                "download of the same bits to the host (what the chain paid before a host deframer could start; the host deframer's\n"
                "own time is not in it), C = rr_bit_decoder over as many f32 symbols (the packet-side yardstick).  P + F counts as slower\n"
                "than D when the medians are apart by at least the sum of the interquartile ranges.\n\n"
                "| shape | bits | frames per push | P ms | launches | P Gbit/s | F ms | P + F ms | D ms | C ms | D / (P + F) | C / P | P + F slower than D |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['bits']:,} | {r['frames_per_push']:,} | {r['P_ms']} ({r['P_iqr_ms']}) | {r['P_launches']} | "
                    f"{r['P_Gbit_per_s']} | {r['F_ms']} ({r['F_iqr_ms']}) | {r['PF_ms']} ({r['PF_iqr_ms']}) | {r['D_ms']} ({r['D_iqr_ms']}) | "
                    f"{r['C_ms']} ({r['C_iqr_ms']}) | {r['D_over_PF']} | {r['C_over_P']} | {'yes' if r['PF_slower_than_D'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
