#!/usr/bin/env python3
"""The KISS blocks (rr_kiss_encode_create, rr_kiss_decode_create) against the host paths they replace, same box, interleaved.

    tools/kiss_probe.py [--steps 20] [--warmup 3] [--out profiles/kiss_probe.md]

Encode, on the frames an rr_hdlc_deframer holds after a push (100,000 packets of 256 bytes: the README's loop-back shape; 64
packets of 256 bytes; one frame of 65,000 bytes, near the deframer's largest max_size).  Before every timed step the deframer is
pushed again and waited for, so both ways start from records and an arena nobody has fetched:
  (E) rr_kiss_encode_frames on the deframer's device arena, rr_kiss_encode_records, and the ONE download of the KISS bytes
  (R) rr_hdlc_frames + rr_hdlc_frame_bytes, then the escaping on one host core (encode_numpy of tests/kiss_model.py)
Decode, on E's output and on 2^24 random bytes, the bytes being in host memory as a socket leaves them:
  (D) rr_kiss_decode_push (the upload included) + rr_kiss_packets: the packets stay on the device for rr_hdlc_framer_push_kiss
  (Dd) rr_kiss_decode_push_dev on bytes already on the device + rr_kiss_packets
  (U) the un-escaping on one host core (decode_numpy) + the upload of the packets' bytes that rr_hdlc_framer_push needs
Reported: the median ms per step with the interquartile range, kernel launches per step, and whether the device way is slower:
it is when its median is behind by at least the sum of the two interquartile ranges.
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
import kiss_model as km  # noqa: E402
import rustradio_amd as rr  # noqa: E402


def launches():
    return int(rr.lib().rr_debug_kernel_launches())


def timed(ways, steps, warmup, before=None):
    """ways: name -> callable; interleaved, synchronised -> name -> (median ms, iqr ms, launches)"""
    times, nl = {k: [] for k in ways}, {}
    for it in range(warmup + steps):
        for k, fn in ways.items():
            if before:
                before()
            torch.cuda.synchronize()
            l0, t0 = launches(), time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            nl[k] = launches() - l0
    out = {}
    for k, t in times.items():
        t = np.asarray(t)
        out[k] = (round(float(np.median(t)), 4), round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4), nl[k])
    return out


def slower(a, b):
    return bool(a[0] - b[0] >= a[1] + b[1])


def decode_row(name, host_kiss, a):
    """D, Dd and U over one KISS stream in host memory"""
    d_kiss = torch.from_numpy(host_kiss).cuda()
    kd, kdd = rr.KissDecode(1 << 20), rr.KissDecode(1 << 20)
    got = {}

    def D():
        if rr.lib().rr_kiss_decode_push(kd._h, host_kiss.ctypes.data, len(host_kiss)) != 0:
            raise RuntimeError(rr.last_error())
        got["D"] = len(kd.packets())

    def Dd():
        kdd.push_dev(d_kiss.data_ptr(), len(host_kiss))
        got["Dd"] = len(kdd.packets())

    def U():
        r = km.decode_numpy(host_kiss, 1 << 20)
        torch.from_numpy(r[4]).cuda() if len(r[4]) else None
        got["U"] = len(r[0])

    t = timed({"D": D, "Dd": Dd, "U": U}, a.steps, a.warmup)
    row = {"shape": name, "kiss_bytes": int(len(host_kiss)), "packets": got["U"], "same_packets": got["D"] == got["Dd"] == got["U"]}
    for k, v in t.items():
        row[k + "_ms"], row[k + "_iqr_ms"], row[k + "_launches"] = v
    row["U_over_D"] = round(row["U_ms"] / row["D_ms"], 2)
    row["D_slower_than_U"] = slower(t["D"], t["U"])
    row["D_GB_per_s"] = round(len(host_kiss) / (row["D_ms"] * 1e-3) / 1e9, 3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kiss_probe.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    shapes = (("64 packets of 256 bytes", 64, 256), ("100,000 packets of 256 bytes", 100_000, 256), ("one frame of 65,000 bytes", 1, 65_000))
    enc_rows, dec_rows = [], []
    for name, P, L in shapes:
        data = rng.integers(0, 256, P * L, dtype=np.uint8)
        lens = np.full(P, L, np.uintp)
        starts = (np.arange(P) * L).astype(np.uintp)
        d_in = torch.from_numpy(data).cuda()
        fr, df, ke = rr.HdlcFramer(rr.FRAME_FCS), rr.HdlcDeframer(0, max(L + 8, 300)), rr.KissEncode()
        cap = fr.bound(lens)
        d_bits = torch.empty(cap, dtype=torch.uint8, device="cuda")
        fr.push_dev(d_in.data_ptr(), len(data), starts, lens, d_bits.data_ptr(), cap)
        n = fr.records()[1]
        out_cap = rr.KissEncode.bound(lens)
        d_kiss = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
        res = {}

        def before():
            df.push_dev(d_bits.data_ptr(), n)          # the same frames again: nothing of them fetched yet
            df.sync()

        def E():
            ke.encode_frames(df, d_kiss.data_ptr(), out_cap)
            res["E"] = d_kiss[:ke.records()[1]].cpu().numpy()

        def R():
            rec, arena = df.frames(), df.frame_bytes()
            res["R"] = km.encode_numpy(arena, rec["start"], rec["len"])

        t = timed({"E": E, "R": R}, a.steps, a.warmup, before)
        row = {"shape": name, "packets": P, "frames": int(len(df.frames())), "kiss_bytes": int(len(res["E"])),
               "E_equals_R": bool(np.array_equal(res["E"], res["R"]))}
        for k, v in t.items():
            row[k + "_ms"], row[k + "_iqr_ms"], row[k + "_launches"] = v
        row["R_over_E"] = round(row["R_ms"] / row["E_ms"], 2)
        row["E_slower_than_R"] = slower(t["E"], t["R"])
        print(json.dumps(row), flush=True)
        enc_rows.append(row)
        dec_rows.append(decode_row("the encoder's output: " + name, np.ascontiguousarray(res["E"]), a))
        del fr, df, ke, d_bits, d_kiss, d_in
        torch.cuda.empty_cache()
    dec_rows.append(decode_row("2^24 random bytes", rng.integers(0, 256, 1 << 24, dtype=np.uint8), a))
    dev = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        f.write("# rr_kiss_encode / rr_kiss_decode: KISS framing on the device against the host paths it replaces\n\n"
                f"`tools/kiss_probe.py --steps {a.steps} --warmup {a.warmup}` on {dev}; host-timed calls, synchronised, interleaved, median\n"
                "over the steps (interquartile range in brackets).  E = rr_kiss_encode_frames on the deframer's device arena +\n"
                "rr_kiss_encode_records + the one download of the KISS bytes; R = rr_hdlc_frames + rr_hdlc_frame_bytes + the escaping in numpy\n"
                "on one host core.  D = rr_kiss_decode_push of host bytes (upload included) + rr_kiss_packets; Dd = the same from device\n"
                "bytes; U = the un-escaping in numpy on one host core + the upload of the packets' bytes.  A way counts as slower than\n"
                "another when its median is behind by at least the sum of the two interquartile ranges.\n\n"
                "## Encode\n\n| shape | frames | KISS bytes | E ms | launches | R ms | R / E | E = R | E slower than R |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in enc_rows:
            f.write(f"| {r['shape']} | {r['frames']:,} | {r['kiss_bytes']:,} | {r['E_ms']} ({r['E_iqr_ms']}) | {r['E_launches']} | "
                    f"{r['R_ms']} ({r['R_iqr_ms']}) | {r['R_over_E']} | {'yes' if r['E_equals_R'] else 'NO'} | {'yes' if r['E_slower_than_R'] else 'no'} |\n")
        f.write("\n## Decode\n\n| stream | KISS bytes | packets | D ms | launches | D GB/s | Dd ms | U ms | U / D | same packets | D slower than U |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in dec_rows:
            f.write(f"| {r['shape']} | {r['kiss_bytes']:,} | {r['packets']:,} | {r['D_ms']} ({r['D_iqr_ms']}) | {r['D_launches']} | {r['D_GB_per_s']} | "
                    f"{r['Dd_ms']} ({r['Dd_iqr_ms']}) | {r['U_ms']} ({r['U_iqr_ms']}) | {r['U_over_D']} | {'yes' if r['same_packets'] else 'NO'} | "
                    f"{'yes' if r['D_slower_than_U'] else 'no'} |\n")
        f.write("\nRows as JSON:\n\n```\n" + "\n".join(json.dumps(r) for r in enc_rows + dec_rows) + "\n```\n")


if __name__ == "__main__":
    main()
