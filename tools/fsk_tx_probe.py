#!/usr/bin/env python3
"""The packet modulator (rr_fsk_tx_create) against the same work done by an output-rate scan and against a plain resampler moving
the same bytes, same box, interleaved, the bits resident in HBM.

    tools/fsk_tx_probe.py [--steps 5] [--warmup 1] [--out profiles/fsk_tx_probe.md]

Shapes (random line bits, every step a further push of the same handle: steady state):
  bell202   AFSK   40:1 then 50:1, 1200 / 2200 Hz, k1 = 2 pi / 48000, gain 0.5, k2 = 2 pi 5000 / 2400000; about 10^8 outputs per
            push (50,000 bits) and 512,000 (256 bits)
  g3ruh     DIRECT 5:1 then 8:1, +-3000, k1 = 2 pi / 48000, gain 0.5; about 10^8 outputs (2,500,000 bits) and 512,000 (12,800 bits)
  1:1 / 1:1 AFSK, 10^8 and 512,000 bits
Per shape, in turn:
  (A) one rr_fsk_tx_push_dev (AFSK: with d_audio), synchronised and host-timed
  (B) AFSK only: rr_fm_tx(I2, D2, k2) over A's audio through rr_block_work_dev until it has taken it all: the second half of A's
      work done by a scan at the OUTPUT rate (A's first half, the audio, is not in B's time)
  (C) the yardstick: rr_resampler(I2, D2) moving the same output bytes (Complex in, Complex out) from a buffer of A's audio length
Reported: launches (rr_debug_kernel_launches), median ms with the interquartile range, outputs per second, B / A and C / A.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rustradio_amd as rr  # noqa: E402

K_AUDIO = 2.0 * math.pi / 48000.0
SHAPES = [
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, (40, 1, 1200.0, 2200.0, K_AUDIO, 0.5, 50, 1, 2.0 * math.pi * 5000.0 / 2400000.0), 50_000),
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, (40, 1, 1200.0, 2200.0, K_AUDIO, 0.5, 50, 1, 2.0 * math.pi * 5000.0 / 2400000.0), 256),
    ("g3ruh 5:1 / 8:1", rr.FSK_TX_DIRECT, (5, 1, -3000.0, 3000.0, K_AUDIO, 0.5, 8, 1, 0.0), 2_500_000),
    ("g3ruh 5:1 / 8:1", rr.FSK_TX_DIRECT, (5, 1, -3000.0, 3000.0, K_AUDIO, 0.5, 8, 1, 0.0), 12_800),
    ("1:1 / 1:1", rr.FSK_TX_AFSK, (1, 1, -1.0, 1.0, 0.3, 0.5, 1, 1, 0.4), 100_000_000),
    ("1:1 / 1:1", rr.FSK_TX_AFSK, (1, 1, -1.0, 1.0, 0.3, 0.5, 1, 1, 0.4), 512_000),
]


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def drain(blk, d_in, n_in, in_es, d_out, cap, out_es):
    """a stream block over a whole device window -> produced"""
    took = out = 0
    while True:
        _, c, p, _ = blk.work_dev(d_in + in_es * took, n_in - took, d_out + out_es * out, cap - out)
        took, out = took + c, out + p
        if c == 0 and p == 0:
            break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsk_tx_probe.md"))
    a = ap.parse_args()
    rows = []
    for name, mode, prm, n_bits in SHAPES:
        afsk = mode == rr.FSK_TX_AFSK
        i2, d2, k2 = prm[6], prm[7], prm[8]
        h = rr.FskTx(mode, *prm)
        na, no = h.count(n_bits)
        g = torch.Generator(device="cuda").manual_seed(n_bits)
        out = torch.empty(no + 8, dtype=torch.complex64, device="cuda")
        aud = torch.empty(na + 8, dtype=torch.float32, device="cuda") if afsk else None
        ref = torch.empty(no + 8, dtype=torch.complex64, device="cuda")
        yin = torch.zeros(na + 8, dtype=torch.complex64, device="cuda")
        fm = rr.FmTx(i2, d2, k2) if afsk else None
        rs = rr.RationalResampler(i2, d2, np.complex64)
        row = {"shape": name, "mode": "AFSK" if afsk else "DIRECT", "bits": n_bits, "audio": na, "outputs": no}
        tA, tB, tC = [], [], []
        for it in range(a.warmup + a.steps):
            bits = torch.randint(0, 2, (n_bits,), generator=g, device="cuda", dtype=torch.uint8)
            timed = it >= a.warmup
            torch.cuda.synchronize()
            l0 = launches()
            t0 = time.perf_counter()
            got = h.push_dev(bits.data_ptr(), n_bits, out.data_ptr(), no + 8, aud.data_ptr() if afsk else 0, na + 8 if afsk else 0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            row["A_launches"] = launches() - l0
            assert got[0] == no                                # (n_bits I1 / D1 and its I2 / D2 are whole numbers in every shape)
            if afsk:
                l0 = launches()
                t2 = time.perf_counter()
                pb = drain(fm, aud.data_ptr(), na, 4, ref.data_ptr(), no + 8, 8)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                row["B_launches"] = launches() - l0
                assert pb == no
                if timed:
                    tB.append((t3 - t2) * 1e3)
            l0 = launches()
            t4 = time.perf_counter()
            pc = drain(rs, yin.data_ptr(), na, 8, ref.data_ptr(), no + 8, 8)
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            row["C_launches"] = launches() - l0
            assert pc == no
            if timed:
                tA.append((t1 - t0) * 1e3)
                tC.append((t5 - t4) * 1e3)
        row["A_ms"], row["A_iqr_ms"] = med(tA)
        row["C_ms"], row["C_iqr_ms"] = med(tC)
        row["A_Gout_per_s"] = round(no / (row["A_ms"] * 1e-3) / 1e9, 2)
        row["C_over_A"] = round(row["C_ms"] / row["A_ms"], 2)
        if afsk:
            row["B_ms"], row["B_iqr_ms"] = med(tB)
            row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del h, fm, rs, out, aud, ref, yin
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_fsk_tx_create: line bits to AFSK / FSK baseband, the bits resident in HBM\n\n"
                f"`tools/fsk_tx_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; ONE run, median over the {a.steps} timed steps\n"
                f"(interquartile range in brackets) after {a.warmup} warm-up step(s), every step a further push of the same handle, all sides\n"
                "interleaved in one process, host-timed and synchronised.  A = one rr_fsk_tx_push_dev (AFSK: with d_audio).  B (AFSK) =\n"
                "rr_fm_tx(I2, D2, k2) over A's audio: the second half of A's work as a scan at the output rate (the audio itself is not in\n"
                "B's time).  C = rr_resampler(I2, D2) moving the same output bytes, the yardstick.  A loss of A against B (B / A below 1)\n"
                "is in bold; C / A below 1 says how far A is from a plain copy at that shape.\n\n"
                "| shape | mode | bits | audio | outputs | A launches | A ms | G outputs/s | B launches | B ms | B / A | C launches | C ms | C / A |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "B_ms" in r:
                ba = f"{r['B_over_A']}" if r["B_over_A"] >= 1 else f"**{r['B_over_A']}**"
                b = f"{r['B_launches']} | {r['B_ms']} ({r['B_iqr_ms']}) | {ba}"
            else:
                b = "- | - | -"
            f.write(f"| {r['shape']} | {r['mode']} | {r['bits']:,} | {r['audio']:,} | {r['outputs']:,} | {r['A_launches']} | "
                    f"{r['A_ms']} ({r['A_iqr_ms']}) | {r['A_Gout_per_s']} | {b} | {r['C_launches']} | {r['C_ms']} ({r['C_iqr_ms']}) | "
                    f"{r['C_over_A']} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows) + "\n```\n")


if __name__ == "__main__":
    main()
