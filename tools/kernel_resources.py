#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS figures from hipcc's device assembly (the .amdhsa metadata block).

    tools/kernel_resources.py [--build DIR] [--diff OLD_DIR] [file.hip ...]
    tools/kernel_resources.py [--build DIR] [--no-build] --loop 'k_fftfilt_os<11, 0, 0>' [--blocks 0-3,7] [file.hip ...]

--build DIR : compile every rustradio_amd/csrc/kernels_*.hip (or the files named) to DIR/<name>.s with the product's flags
              (device only, no GPU needed) and print one line per kernel: VGPRs, AGPRs, SGPRs, spilled VGPRs, scratch bytes
--diff OLD  : print only the kernels whose figures differ from OLD/<name>.s (a build of another revision)

--loop NAME : instruction histogram of the tile loop of the kernel whose demangled name contains NAME: the loop (a backward
              branch and its target) that holds the most packed-f32 instructions, innermost on a tie.  One line per basic block
              of the loop and the sum; --blocks sums a chosen subset instead (block numbers as printed), which is how the
              steady-state path is counted apart from the boundary-tile blocks that sit in the same loop.
--spans N   : with --loop: every backward-branch span of that kernel with exactly N global stores, one line each (-1: all
              spans with packed math) — the per-row0 interior loops of k_fftfilt_os are nested in the loop --loop picks
--no-build  : read DIR/<name>.s as it is

A tile kernel that starts to spill is 1.5-2x slower (every scratch access waits on the whole in-order vmcnt queue,
profiles/TUNING_LOG.md §4.1), so every change to a kernel is checked with this before it goes to the GPU.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rustradio_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-S"]
NO_SLP = {"kernels_fft.hip", "kernels_poly.hip"}


def build(files, out, extra):
    os.makedirs(out, exist_ok=True)
    procs = []
    for f in files:
        name = os.path.basename(f)
        cmd = ["hipcc"] + FLAGS + (["-fno-slp-vectorize"] if name in NO_SLP else []) + extra + \
              ["-o", os.path.join(out, name.replace(".hip", ".s")), f]
        procs.append((name, subprocess.Popen(cmd, cwd=CSRC, stderr=subprocess.PIPE)))
    for name, p in procs:
        _, err = p.communicate()
        if p.returncode:
            sys.exit(f"{name}: {err.decode()[-2000:]}")


def parse(path):
    """-> {demangled-ish kernel name: (vgpr, agpr, sgpr, vgpr_spill, scratch, lds)}"""
    txt = open(path, errors="replace").read()
    out = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        def g(key):
            m = re.search(r"\." + key + r":\s+(\S+)", blk)
            return m.group(1) if m else "0"
        name = g("name")
        agpr = blk.split("\n", 1)[0].strip()
        out[name] = tuple(int(x) for x in (g("vgpr_count"), agpr, g("sgpr_count"), g("vgpr_spill_count"),
                                             g("private_segment_fixed_size"), g("group_segment_fixed_size")))
    return out


CLASSES = ["pk_f32", "lds", "gload", "gstore", "flat", "wait_sync", "s_nop", "lane", "valu_addr64", "valu_other", "exec", "branch", "salu_other"]


def classify(ins, ops):
    if ins.startswith("v_pk_"):
        return "pk_f32"
    if ins.startswith("ds_"):
        return "lds"
    if ins.startswith(("global_load", "buffer_load", "scratch_load")):
        return "gload"
    if ins.startswith(("global_store", "global_atomic", "buffer_store", "scratch_store")):
        return "gstore"
    if ins.startswith("flat_"):
        return "flat"
    if ins in ("s_waitcnt", "s_barrier", "s_setprio"):
        return "wait_sync"
    if ins == "s_nop":
        return "s_nop"
    if ins.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if ins.startswith(("v_add_co", "v_addc", "v_sub_co", "v_subb", "v_lshl_add_u64", "v_lshlrev_b64", "v_mad_u64", "v_mad_i64")):
        return "valu_addr64"
    if ins.startswith("v_"):
        return "valu_other"
    if ins.startswith(("s_cbranch", "s_branch", "s_swappc", "s_setpc", "s_endpgm")):
        return "branch"
    if "saveexec" in ins or re.search(r"\bexec\b", ops):
        return "exec"
    return "salu_other"


def kernel_body(txt, mangled):
    m = re.search(r"^" + re.escape(mangled) + r":.*$", txt, re.M)
    end = txt.index(".Lfunc_end", m.end())
    return txt[m.end():end].split("\n")


def tile_loop(lines):
    """-> (first, last) line indices of the backward-branch span holding the most v_pk_ instructions (innermost on a tie)"""
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    pk = [0]
    for ln in lines:
        pk.append(pk[-1] + (ln.strip().startswith("v_pk_")))
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and label_at.get(m.group(1), i + 1) <= i:
            j = label_at[m.group(1)]
            key = (pk[i + 1] - pk[j], -(i - j))
            if best is None or key > best[0]:
                best = (key, j, i)
    if best is None:
        sys.exit("no loop in this kernel")
    return best[1], best[2]


def parse_blocks(sel):
    out = set()
    for part in sel.split(","):
        a, _, b = part.partition("-")
        out.update(range(int(a), int(b or a) + 1))
    return out


def span_report(lines, stores, title):
    """every backward-branch span of the kernel that holds packed math and exactly `stores` global stores (all of them
    when stores < 0), counted line by line: the per-row0 interior loops of k_fftfilt_os are such spans, nested in the
    edge-tile loop that --loop alone reports"""
    label_at = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    print(title, "- backward-branch spans" + (f" with {stores} global stores" if stores >= 0 else ""))
    for i, ln in enumerate(lines):
        m = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if not m or label_at.get(m.group(1), i + 1) > i:
            continue
        h = dict.fromkeys(CLASSES, 0)
        for t in (x.split(";")[0].strip() for x in lines[label_at[m.group(1)]:i + 1]):
            if t and not t.startswith(".") and not t.startswith(";"):
                ins, _, ops = t.partition(" ")
                h[classify(ins, ops)] += 1
        if h["pk_f32"] and (stores < 0 or h["gstore"] == stores):
            print(f"{m.group(1):12s} " + " ".join(f"{c}={v}" for c, v in h.items() if v) + f" total={sum(h.values())}")


def loop_report(path, want, blocks, stores=None):
    txt = open(path, errors="replace").read()
    names = list(parse(path))
    dm = demangle(names)
    hits = [k for k in names if want in dm[k]]
    if len(hits) != 1:
        sys.exit(f"{want!r} matches {len(hits)} kernels of {os.path.basename(path)}: " + ", ".join(re.sub(r"\(.*", "", dm[k]) for k in hits[:8]))
    lines = kernel_body(txt, hits[0])
    if stores is not None:
        return span_report(lines, stores, re.sub(r"\(.*", "", dm[hits[0]]).replace("void rr::", ""))
    lo, hi = tile_loop(lines)
    # the loop's blocks: the header and every block the compiler marks "in Loop: Header=<it>" (some are laid out behind the
    # backward branch), blocks of loops nested in it included
    hm = re.search(r"Header=(BB\d+_\d+) ", lines[lo])       # (the branch target may be the latch, laid out before the header)
    hdr = hm.group(1) if hm else re.match(r"^\.L(BB\d+_\d+):", lines[lo]).group(1)
    rows, cur, detail = [], None, {}
    for k, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.(\d+):", ln)
        if m:
            inside = k == lo or ("Header=" + hdr + " ") in ln or ln.startswith(".L" + hdr + ":") or (lo <= k <= hi and "Header=" in ln)
            cur = [m.group(1) or "%bb." + m.group(2), dict.fromkeys(CLASSES, 0)] if inside else None
            if inside:
                rows.append(cur)
            continue
        t = ln.split(";")[0].strip()
        if not t or t.startswith(".") or cur is None:
            continue
        ins, _, ops = t.partition(" ")
        c = classify(ins, ops)
        cur[1][c] += 1
        if blocks is None or len(rows) - 1 in blocks:
            detail[ins] = detail.get(ins, 0) + 1
    print(re.sub(r"\(.*", "", dm[hits[0]]).replace("void rr::", ""), "- tile loop,", len(rows), "basic blocks")
    print(f"{'#':>3s} {'block':12s} " + " ".join(f"{c:>11s}" for c in CLASSES) + f" {'total':>6s}")
    tot = dict.fromkeys(CLASSES, 0)
    for i, (lab, h) in enumerate(rows):
        if blocks is not None and i not in blocks:
            continue
        print(f"{i:3d} {lab:12s} " + " ".join(f"{h[c]:11d}" for c in CLASSES) + f" {sum(h.values()):6d}")
        for c in CLASSES:
            tot[c] += h[c]
    print(f"{'':3s} {'sum':12s} " + " ".join(f"{tot[c]:11d}" for c in CLASSES) + f" {sum(tot.values()):6d}")
    print("by mnemonic: " + ", ".join(f"{k} {v}" for k, v in sorted(detail.items(), key=lambda kv: (-kv[1], kv[0]))))


def demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            p = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
            return dict(zip(names, p.stdout.split("\n")))
        except Exception:
            continue
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="/tmp/rr_kres")
    ap.add_argument("--diff", default=None)
    ap.add_argument("--extra", default="", help="extra compiler flags, e.g. -DRR_POLY_NB=2")
    ap.add_argument("--loop", default=None, help="demangled kernel name (substring): histogram of its tile loop")
    ap.add_argument("--blocks", default=None, help="with --loop: sum only these basic blocks, e.g. 0-3,7")
    ap.add_argument("--spans", type=int, default=None, metavar="N",
                    help="with --loop: one line per backward-branch span of the kernel that holds exactly N global stores "
                         "(-1: every span with packed math) instead of the one loop --loop picks")
    ap.add_argument("--no-build", action="store_true", help="use the assembly already in --build DIR")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = [os.path.abspath(f) for f in a.files] or sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("kernels_") and f.endswith(".hip"))
    if not a.no_build:
        build(files, a.build, a.extra.split())
    if a.loop:
        for f in files:
            sp = os.path.join(a.build, os.path.basename(f).replace(".hip", ".s"))
            if any(a.loop in v for v in demangle(list(parse(sp))).values()):
                return loop_report(sp, a.loop, parse_blocks(a.blocks) if a.blocks else None, a.spans)
        sys.exit(f"no kernel named like {a.loop!r}")
    bad = 0
    for f in files:
        sname = os.path.basename(f).replace(".hip", ".s")
        new = parse(os.path.join(a.build, sname))
        old = parse(os.path.join(a.diff, sname)) if a.diff and os.path.exists(os.path.join(a.diff, sname)) else None
        dm = demangle(list(new))
        for k, v in sorted(new.items(), key=lambda kv: dm[kv[0]]):
            if old is not None and old.get(k) == v:
                continue
            label = re.sub(r"\(.*", "", dm[k]).replace("void rr::", "")
            was = f"   was {old[k]}" if old is not None and k in old else ("   (new)" if old is not None else "")
            flag = "  <-- SPILLS" if v[3] or v[4] else ""
            bad += bool(v[3] or v[4])
            print(f"{label:70s} vgpr {v[0]:3d} agpr {v[1]:3d} sgpr {v[2]:3d} spill {v[3]:3d} scratch {v[4]:4d} B{was}{flag}")
    print(f"{bad} kernels with spills / scratch" if bad else "no kernel spills")


if __name__ == "__main__":
    main()
