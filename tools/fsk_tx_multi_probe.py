#!/usr/bin/env python3
"""N packet modulators behind one handle (rr_fsk_tx_multi_create) against the path it replaces, N rr_fsk_tx handles with one push
each, same box, interleaved, the bits resident in HBM; and framer -> modulator for one stream with and without the host read.

    tools/fsk_tx_multi_probe.py [--steps 5] [--warmup 1] [--out profiles/fsk_tx_multi_probe.md]

Shapes (random line bits, every stream full, every step a further push of the same handles: steady state):
  bell202   AFSK   40:1 then 50:1, 1200 / 2200 Hz, k1 = 2 pi / 48000, gain 0.5, k2 = 2 pi 5000 / 2400000 (2,000 outputs per bit):
            256 x 5,000 bits, 4,096 x 256 bits, 32 x 50,000 bits, 1 x 50,000 bits
  g3ruh     DIRECT 5:1 then 8:1, +-3000, k1 = 2 pi / 48000, gain 0.5 (40 outputs per bit): 256 x 50,000 bits
A shape whose nstreams * out_cap is above 2^30 is refused by rr_fsk_tx_multi_push_dev; the refusal is recorded and the shape is
measured with the most bits per stream (a round number) that fit.
Per shape, in turn:
  (A) one rr_fsk_tx_multi_push_dev (AFSK: with d_audio; d_counts on the device, every count full), synchronised and host-timed
  (B) N rr_fsk_tx_push_dev, one per handle, into the same buffers, from one Python loop, then one synchronise
Reported: launches (rr_debug_kernel_launches), median ms with the interquartile range, outputs per second of A, B / A.
Then HdlcFramer(FCS | NRZI) over 8 packets of 200 bytes -> bell202:
  (R) framer push, rr_hdlc_framer_records (the host read: it waits), rr_fsk_tx_push_dev of exactly the produced bits
  (D) framer push, rr_fsk_tx_multi_push_dev(nstreams 1) with d_counts = rr_hdlc_framer_produced_dev and n_cap = the framer's bound
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
BELL = (40, 1, 1200.0, 2200.0, K_AUDIO, 0.5, 50, 1, 2.0 * math.pi * 5000.0 / 2400000.0)
G3RUH = (5, 1, -3000.0, 3000.0, K_AUDIO, 0.5, 8, 1, 0.0)
# name, mode, parameters, nstreams, bits per stream as asked for, bits per stream that fit 2^30 outputs in all
SHAPES = [
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, BELL, 256, 5_000, 2_000),
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, BELL, 4096, 256, 128),
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, BELL, 32, 50_000, 16_000),
    ("bell202 40:1 / 50:1", rr.FSK_TX_AFSK, BELL, 1, 50_000, 50_000),
    ("g3ruh 5:1 / 8:1", rr.FSK_TX_DIRECT, G3RUH, 256, 50_000, 50_000),
]


def med(t):
    t = np.asarray(t)
    return round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def refusal(h, n_bits):
    """what rr_fsk_tx_multi_push_dev says to a push of n_bits per stream (said before any device is touched) or None"""
    ac, oc = h.bound(n_bits)
    some = torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if h.nstreams * oc <= 1 << 30 and h.nstreams * ac <= 1 << 30:
        return None
    try:
        h.push_dev(some.data_ptr(), n_bits, n_bits, None, some.data_ptr(), oc, 0, 0)
    except ValueError as e:
        return str(e)
    raise AssertionError("a push above 2^30 outputs was not refused")


def shape_row(name, mode, prm, N, asked, n_bits, steps, warmup):
    afsk = mode == rr.FSK_TX_AFSK
    hm = rr.FskTxMulti(N, mode, *prm)
    row = {"shape": name, "mode": "AFSK" if afsk else "DIRECT", "streams": N, "bits_asked": asked, "bits": n_bits}
    said = refusal(hm, asked)
    if said is not None:
        row["asked_refused"] = said
    else:
        assert asked == n_bits
    ac, oc = hm.bound(n_bits)
    ones = [rr.FskTx(mode, *prm) for _ in range(N)]
    assert ones[0].count(n_bits) == (ac, oc)   # (n_bits I1 / D1 and its I2 / D2 are whole numbers in every shape: no residues)
    row["audio"], row["outputs"] = N * ac, N * oc
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + n_bits)
    out = torch.empty((N, oc), dtype=torch.complex64, device="cuda")
    aud = torch.empty((N, ac), dtype=torch.float32, device="cuda") if afsk else None
    counts = torch.full((N,), n_bits, dtype=torch.int64, device="cuda")
    tA, tB = [], []
    for it in range(warmup + steps):
        bits = torch.randint(0, 2, (N, n_bits), generator=g, device="cuda", dtype=torch.uint8)
        torch.cuda.synchronize()
        l0 = launches()
        t0 = time.perf_counter()
        hm.push_dev(bits.data_ptr(), n_bits, n_bits, counts.data_ptr(), out.data_ptr(), oc, aud.data_ptr() if afsk else 0, ac if afsk else 0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        row["A_launches"] = launches() - l0
        pb, po, pa = bits.data_ptr(), out.data_ptr(), aud.data_ptr() if afsk else 0
        l0 = launches()
        t2 = time.perf_counter()
        for c, h in enumerate(ones):
            h.push_dev(pb + c * n_bits, n_bits, po + 8 * c * oc, oc, pa + 4 * c * ac if afsk else 0, ac if afsk else 0)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        row["B_launches"] = launches() - l0
        if it >= warmup:
            tA.append((t1 - t0) * 1e3)
            tB.append((t3 - t2) * 1e3)
    made = hm.counts()
    assert bool((made[:, 0] == ac).all()) and bool((made[:, 1] == oc).all())
    row["A_ms"], row["A_iqr_ms"] = med(tA)
    row["B_ms"], row["B_iqr_ms"] = med(tB)
    row["A_Gout_per_s"] = round(N * oc / (row["A_ms"] * 1e-3) / 1e9, 2)
    row["B_over_A"] = round(row["B_ms"] / row["A_ms"], 2)
    return row


def framer_row(steps, warmup):
    flags = rr.FRAME_FCS | rr.FRAME_NRZI
    rng = np.random.default_rng(5)
    lens = np.full(8, 200, np.uintp)
    starts = (np.cumsum(lens) - lens).astype(np.uintp)
    fr_r, fr_d = rr.HdlcFramer(flags), rr.HdlcFramer(flags)
    cap = fr_r.bound(lens)
    one = rr.FskTx(rr.FSK_TX_AFSK, *BELL)
    mul = rr.FskTxMulti(1, rr.FSK_TX_AFSK, *BELL)
    ac, oc = mul.bound(cap)
    d_bits = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out = torch.empty(oc, dtype=torch.complex64, device="cuda")
    aud = torch.empty(ac, dtype=torch.float32, device="cuda")
    row = {"packets": len(lens), "bytes": int(lens.sum()), "bound_bits": cap}
    tR, tD = [], []
    for it in range(warmup + steps):
        d_bytes = torch.from_numpy(rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)).cuda()
        torch.cuda.synchronize()
        l0 = launches()
        t0 = time.perf_counter()
        fr_r.push_dev(d_bytes.data_ptr(), int(lens.sum()), starts, lens, d_bits.data_ptr(), cap)
        n = fr_r.records()[1]                  # the host read
        one.push_dev(d_bits.data_ptr(), n, out.data_ptr(), oc, aud.data_ptr(), ac)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        row["R_launches"], row["bits"] = launches() - l0, n
        l0 = launches()
        t2 = time.perf_counter()
        fr_d.push_dev(d_bytes.data_ptr(), int(lens.sum()), starts, lens, d_bits.data_ptr(), cap)
        mul.push_dev(d_bits.data_ptr(), cap, cap, fr_d.produced_dev(), out.data_ptr(), oc, aud.data_ptr(), ac)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        row["D_launches"] = launches() - l0
        assert int(mul.counts()[0, 0]) == 40 * n
        if it >= warmup:
            tR.append((t1 - t0) * 1e3)
            tD.append((t3 - t2) * 1e3)
    row["R_ms"], row["R_iqr_ms"] = med(tR)
    row["D_ms"], row["D_iqr_ms"] = med(tD)
    row["R_over_D"] = round(row["R_ms"] / row["D_ms"], 2)
    return row


def bold_if_loss(ratio):
    return f"{ratio}" if ratio >= 1 else f"**{ratio}**"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsk_tx_multi_probe.md"))
    a = ap.parse_args()
    rows = []
    for name, mode, prm, N, asked, n_bits in SHAPES:
        row = shape_row(name, mode, prm, N, asked, n_bits, a.steps, a.warmup)
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    fr = framer_row(a.steps, a.warmup)
    print(json.dumps(fr), flush=True)
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_fsk_tx_multi_create: N packet modulators behind one handle, the bits resident in HBM\n\n"
                f"`tools/fsk_tx_multi_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; ONE run, median over the {a.steps} timed steps\n"
                f"(interquartile range in brackets) after {a.warmup} warm-up step(s), every step a further push of the same handles, all sides\n"
                "interleaved in one process, host-timed (Python, ctypes) and synchronised.  A = one rr_fsk_tx_multi_push_dev (AFSK: with\n"
                "d_audio; the counts read on the device, every stream full).  B = the path it replaces: N rr_fsk_tx handles, one\n"
                "rr_fsk_tx_push_dev each from one loop, then one synchronise.  A loss of A (B / A below 1) is in bold.  `bits asked` is\n"
                "the shape as it was asked for; where nstreams x out_cap is above 2^30 the push is refused and `bits` is what was measured.\n\n"
                "| shape | mode | streams | bits asked | bits | outputs | A launches | A ms | G outputs/s | B launches | B ms | B / A |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['mode']} | {r['streams']:,} | {r['bits_asked']:,} | {r['bits']:,} | {r['outputs']:,} | "
                    f"{r['A_launches']} | {r['A_ms']} ({r['A_iqr_ms']}) | {r['A_Gout_per_s']} | {r['B_launches']} | "
                    f"{r['B_ms']} ({r['B_iqr_ms']}) | {bold_if_loss(r['B_over_A'])} |\n")
        f.write("\nframer -> modulator, one stream (HdlcFramer(FCS | NRZI), 8 packets of 200 bytes, bell202).  R = framer push,\n"
                "rr_hdlc_framer_records (the host read), rr_fsk_tx_push_dev of the produced bits.  D = framer push,\n"
                "rr_fsk_tx_multi_push_dev(1 stream) with d_counts = rr_hdlc_framer_produced_dev and n_cap = the framer's bound.  A loss\n"
                "of D (R / D below 1) is in bold.\n\n"
                "| packets | bytes | bits | bound | R launches | R ms | D launches | D ms | R / D |\n|---|---|---|---|---|---|---|---|---|\n"
                f"| {fr['packets']} | {fr['bytes']:,} | {fr['bits']:,} | {fr['bound_bits']:,} | {fr['R_launches']} | {fr['R_ms']} ({fr['R_iqr_ms']}) | "
                f"{fr['D_launches']} | {fr['D_ms']} ({fr['D_iqr_ms']}) | {bold_if_loss(fr['R_over_D'])} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in rows + [fr]) + "\n```\n")


if __name__ == "__main__":
    main()
