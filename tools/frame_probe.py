#!/usr/bin/env python3
"""The fused HDLC framer (rr_hdlc_framer_create) against what exists without it, same box, interleaved, buffers resident in HBM.

    tools/frame_probe.py [--steps 20] [--warmup 3] [--host-steps 3] [--out profiles/frame_probe.md]

The shape is the front of examples/g3ruh.rs:250-267: FcsAdder -> HdlcFramer -> PduToStream -> Scrambler::g3ruh -> NrziEncode, on
64 and on 100,000 packets of 256 random bytes and on one all-0xff packet of 1 MB (the most stuffed bits a payload can have, and a
CRC that must not be one lane's loop).  Four ways, in turn (A, B, C, A, ...):
  (A) rr_hdlc_framer with FCS, G3RUH and NRZI: one handle
  (B) rr_hdlc_framer with FCS alone -> rr_scrambler_g3ruh -> rr_nrzi_encode through device buffers (the count of framed bits is
      read back in between, as a graph would have to)
  (C) rr_quaddemod over as many Complex samples as A writes bits: the yardstick of the other probes
  (H) the closed form of tests/frame_model.py in numpy on one host core, plus the upload of its bits.  Its CRC is a Python loop
      per bit, so at more than 1,000 packets H is timed on the first 1,000 and scaled by the packet count; --host-steps steps.
One step = one push (A), one push and two work_dev() calls (B) or one work_dev() call (C), synchronised, handles kept (every step
is the next stretch of one stream).  Reported: the median ms per step with the interquartile range, kernel launches per step,
whether A's output equals B's, and whether A is slower than B or C: it is when its median is behind by at least the sum of the two
interquartile ranges.
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
import frame_model as fm  # noqa: E402
import rustradio_amd as rr  # noqa: E402

H_MAX = 1000


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    shapes = (("64 packets of 256 bytes", rng.integers(0, 256, 64 * 256, dtype=np.uint8), 64, 256),
              ("100,000 packets of 256 bytes", rng.integers(0, 256, 100_000 * 256, dtype=np.uint8), 100_000, 256),
              ("one all-0xff packet of 1 MB", np.full(1 << 20, 0xff, np.uint8), 1, 1 << 20))
    rows = []
    for name, data, P, L in shapes:
        lens = np.full(P, L, np.uintp)
        starts = (np.arange(P) * L).astype(np.uintp)
        d_in = torch.from_numpy(data).cuda()
        fa = rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI)
        fb, sb, nb = rr.HdlcFramer(rr.FRAME_FCS), rr.Scrambler.g3ruh(), rr.NrziEncode()
        qd = rr.QuadratureDemod(1.0)
        cap = fa.bound(lens)
        ya, yb, b1, b2 = (torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(4))
        fa.push_dev(d_in.data_ptr(), len(data), starts, lens, ya.data_ptr(), cap)
        n = fa.records()[1]                                    # the framed bits of one step: the window of C
        z = torch.view_as_complex(torch.randn(n, 2, dtype=torch.float32, device="cuda"))
        yc = torch.empty(n, dtype=torch.float32, device="cuda")

        def step(k):
            if k == "A":
                fa.push_dev(d_in.data_ptr(), len(data), starts, lens, ya.data_ptr(), cap)
                return n
            if k == "B":
                fb.push_dev(d_in.data_ptr(), len(data), starts, lens, b1.data_ptr(), cap)
                m = fb.records()[1]
                sb.work_dev(b1.data_ptr(), m, b2.data_ptr(), m)
                return nb.work_dev(b2.data_ptr(), m, yb.data_ptr(), m)[2]
            return qd.work_dev(z.data_ptr(), n, yc.data_ptr(), n)[2] + 1

        step("B")                                              # B's stream in step with A's
        torch.cuda.synchronize()
        times = {"A": [], "B": [], "C": []}
        nl = {}
        for it in range(a.warmup + a.steps):
            for k in times:
                torch.cuda.synchronize()
                l0, t0 = launches(), time.perf_counter()
                p = step(k)
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                nl[k] = launches() - l0
                assert p == n, (k, p, n)
        same = bool(torch.equal(ya[:n], yb[:n]))
        # H: the closed form on one host core, and its bits uploaded
        hp = min(P, H_MAX)
        packets = [data[i * L:(i + 1) * L].tobytes() for i in range(hp)]
        th = []
        for it in range(1 + a.host_steps):
            t0 = time.perf_counter()
            bits = fm.closed_form(packets, fm.FCS | fm.G3RUH | fm.NRZI)[0]
            torch.from_numpy(bits).cuda()
            torch.cuda.synchronize()
            if it >= 1:
                th.append((time.perf_counter() - t0) * 1e3 * P / hp)
        row = {"shape": name, "packets": P, "framed_bits": int(n), "A_equals_B": same, "H_scaled_from_packets": hp}
        times["H"] = th
        for k in times:
            t = np.asarray(times[k])
            row[k + "_ms"] = round(float(np.median(t)), 4)
            row[k + "_iqr_ms"] = round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)
            if k != "H":
                row[k + "_launches"] = nl[k]
        row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        row["C_over_A"] = round(row["C_ms"] / row["A_ms"], 2)
        row["H_over_A"] = round(row["H_ms"] / row["A_ms"], 1)
        row["A_Gbit_per_s"] = round(n / (row["A_ms"] * 1e-3) / 1e9, 2)
        row["A_slower_than_B"] = bool(row["A_ms"] - row["B_ms"] >= row["A_iqr_ms"] + row["B_iqr_ms"])
        row["A_slower_than_C"] = bool(row["A_ms"] - row["C_ms"] >= row["A_iqr_ms"] + row["C_iqr_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del fa, fb, sb, nb, qd, ya, yb, b1, b2, z, yc, d_in
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_hdlc_framer_create: FcsAdder -> HdlcFramer -> PduToStream -> Scrambler::g3ruh -> NrziEncode as one block\n\n"
                f"`tools/frame_probe.py --steps {a.steps} --warmup {a.warmup} --host-steps {a.host_steps}` on {dev}; host-timed calls,\n"
                "synchronised, median over the steps (interquartile range in brackets).  A = rr_hdlc_framer(FCS | G3RUH | NRZI), B =\n"
                "rr_hdlc_framer(FCS) -> rr_scrambler_g3ruh -> rr_nrzi_encode through device buffers, C = rr_quaddemod over as many Complex\n"
                "samples as A writes bits (the yardstick: one pass at 12 B per sample), H = the closed form of tests/frame_model.py in\n"
                f"numpy on one host core plus the upload (beyond {H_MAX:,} packets: timed on {H_MAX:,} and scaled).  A counts as slower than\n"
                "another way when its median is behind by at least the sum of the two interquartile ranges.\n\n"
                "| shape | framed bits | A ms | launches | A Gbit/s | B ms | launches | C ms | launches | H ms | B / A | C / A | H / A | A = B | A slower than B | A slower than C |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['framed_bits']:,} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_launches']} | {r['A_Gbit_per_s']} | "
                    f"{r['B_ms']} ({r['B_iqr_ms']}) | {r['B_launches']} | {r['C_ms']} ({r['C_iqr_ms']}) | {r['C_launches']} | "
                    f"{r['H_ms']} ({r['H_iqr_ms']}) | {r['B_over_A']} | {r['C_over_A']} | {r['H_over_A']} | {'yes' if r['A_equals_B'] else 'NO'} | "
                    f"{'yes' if r['A_slower_than_B'] else 'no'} | {'yes' if r['A_slower_than_C'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
