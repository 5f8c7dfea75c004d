"""No GPU: the sequential models of tests/pdu_model.py against the reference's own StreamToPdu vectors and against each other, the
two statements of Midpointer, the host-only logic of the record path under the host sanitizers, and the errors rr.StreamToPdu
reports without a device."""
import json
import os
import subprocess

import numpy as np
import pytest

import pdu_model as pm
import rustradio_amd as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "stream_to_pdu_known_answers.json")))


@pytest.mark.parametrize("name", ["single", "size", "ended_too_soon", "it_ends_with_both", "tags_in_tail", "mid_pdu", "just_end"])
def test_reference_vectors_against_the_sequential_model(name):
    cases = [c for c in VECTORS["cases"] if c["name"] == name]
    assert cases
    for c in cases:
        m = pm.StreamToPduSeq(c["max_size"], c["tail"])
        got = [p for _, p in m.work(VECTORS["samples"], [(p, v) for p, v in c["tags"]])]
        assert got == c["want"], c
        # ... and fed one sample per work() call
        m = pm.StreamToPduSeq(c["max_size"], c["tail"])
        got = []
        for i, s in enumerate(VECTORS["samples"]):
            got += [p for _, p in m.work([s], [(0, v) for p, v in c["tags"] if p == i])]
        assert got == c["want"], c


def test_vector_counts():
    n = {}
    for c in VECTORS["cases"]:
        n[c["name"]] = n.get(c["name"], 0) + 1
    assert n == {"single": 17, "size": 22, "ended_too_soon": 3, "it_ends_with_both": 1, "tags_in_tail": 7, "mid_pdu": 1, "just_end": 1}


def as_plain(per):
    return [[(f, [float(v) for v in p]) for f, p in w] for w in per]


def test_closed_form_equals_the_machine_on_drawn_streams():
    """tail 0..5, max_size 0..12, dense and sparse triggers, up to three cuts (empty windows included)"""
    rng = np.random.default_rng(7)
    npdus = 0
    for _ in range(4000):
        n = int(rng.integers(1, 48))
        trig = (rng.random(n) < rng.choice([0.15, 0.5, 0.85])).astype(F32)
        x = np.arange(n, dtype=F32)
        ms, tl = int(rng.integers(0, 13)), int(rng.integers(0, 6))
        sp = sorted(set(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 4)))))
        a = as_plain(pm.stream_to_pdu_seq(x, trig, 0.5, ms, tl, sp))
        b = as_plain(pm.closed_form_windows(x, trig, 0.5, ms, tl, sp))
        assert a == b, (n, trig, ms, tl, sp)
        npdus += sum(len(w) for w in a)
    assert npdus > 4000


def test_the_split_does_not_change_the_pdus():
    rng = np.random.default_rng(8)
    trig = (rng.random(300) < 0.5).astype(F32)
    x = rng.standard_normal(300).astype(F32)
    whole = [p for w in as_plain(pm.stream_to_pdu_seq(x, trig, 0.5, 9, 2)) for p in w]
    for sp in ([1], [150], [299], [10, 11, 12], list(range(1, 300))):
        assert [p for w in as_plain(pm.stream_to_pdu_seq(x, trig, 0.5, 9, 2, sp)) for p in w] == whole


def test_nan_trigger_and_nan_threshold():
    t = np.array([0, 1, np.nan, 1, 0], F32)
    assert pm.burst_tags(t, 0.5)[0] == [(1, True), (2, False), (3, True), (4, False)]
    assert pm.burst_tags(t, np.nan)[0] == []
    r, f = pm.edges_of(t, 0.5)
    assert list(r) == [1, 3] and list(f) == [2, 4]


def test_midpointer_two_statements_on_noisy_nrz():
    """The reference (f32 sum in order) against the block (exact sum, two ranks).  Where no sample lies between the two means the
    partitions are the same sets and the offsets must be equal bit for bit; only a burst with a sample between the means may
    be left out, and at most 1 % of them."""
    rng = np.random.default_rng(11)
    left_out, total = 0, 600
    for _ in range(total):
        n = int(rng.integers(200, 4000))
        v = pm.noisy_nrz_burst(rng, n, rng.uniform(3.0, 9.0), rng.uniform(-2.0, 2.0), rng.uniform(0.02, 0.3))
        mr, off = pm.midpointer_ref(v)
        blk = pm.midpointer_block(v)
        lo, hi = min(mr, blk["mean"]), max(mr, blk["mean"])
        if np.any((v > lo) & ~(v > hi)):
            left_out += 1
            continue
        assert off is not None and blk["ok"] == 1
        assert F32(off).view(np.uint32) == F32(blk["mid"]).view(np.uint32), (n, off, blk)
    assert left_out <= total // 100, left_out


def test_midpointer_block_statement_equals_partition_and_sorts():
    """from ONE mean, the two ranks of the total order are the reference's two medians (no NaN in the burst)"""
    rng = np.random.default_rng(12)
    for _ in range(200):
        n = int(rng.integers(2, 60))
        v = rng.choice(np.array([-np.inf, -2.5, -0.0, 0.0, 1e-40, 1.0, 3.0, np.inf], F32), n).astype(F32)
        mean = pm.mean_exact(v)
        blk = pm.midpointer_block(v, mean)
        if np.isnan(mean):
            assert blk["ok"] == 0 and blk["nlow"] == n
            continue
        a, b = pm.total_sort(v[v > mean]), pm.total_sort(v[~(v > mean)])
        if len(a) == 0 or len(b) == 0:
            assert blk["ok"] == 0
            continue
        assert blk["ok"] == 1 and blk["nlow"] == len(b)
        assert blk["low"].view(np.uint32) == b[len(b) // 2].view(np.uint32)
        assert blk["high"].view(np.uint32) == a[len(a) // 2].view(np.uint32)


def test_total_order_key():
    v = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], F32)
    v = np.concatenate([v, (-np.array([np.nan], F32))])
    s = pm.total_sort(v)
    assert np.signbit(s[0]) and np.isnan(s[0]) and np.isnan(s[-1]) and not np.signbit(s[-1])
    assert list(s[1:-1]) == [-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf] and np.signbit(s[3]) and not np.signbit(s[4])


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """clamping to cap, the filter by ok, the geometry checks and the pack plan, as a stand-alone program built with
    -fsanitize=address,undefined (rustradio_amd/csrc/pdu_host.hpp compiles without HIP)"""
    exe = str(tmp_path / "test_pdu_hostlogic")
    src = os.path.join(ROOT, "tests", "cpp", "test_pdu_hostlogic.cpp")
    # (the sanitizer runtimes are linked into the program itself: it runs the same whatever else the process loads)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("pdu host logic ok")


def test_symbols_and_record_layout():
    import ctypes
    from rustradio_amd._lib import SYMBOLS
    for s in ("rr_stream_to_pdu_create", "rr_stream_to_pdu_push_dev", "rr_stream_to_pdu_push", "rr_pdu_records", "rr_pdu_edges",
              "rr_pdu_arena_dev", "rr_pdu_fetch", "rr_debug_pdu_ranks", "rr_wpcr_process_pdus", "rr_wpcr_pack_dev"):
        assert s in SYMBOLS and hasattr(ctypes.CDLL(rr.LIB_PATH), s)
    assert rr.PDU_RECORD.itemsize == 48 and rr.PDU_RECORD.fields["nlow"][1] == 40 and rr.PDU_RECORD.fields["mid"][1] == 32


def test_max_size_error_comes_before_any_device():
    with pytest.raises(ValueError, match="max_size beyond 512000 samples"):
        rr.StreamToPdu(0.5, 512001, 0)
    with pytest.raises(ValueError, match="unknown stream_to_pdu flags"):
        rr.StreamToPdu(0.5, 10, 0, flags=2)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert rr.StreamToPdu(0.5, 10, 0).name != ""
    else:
        with pytest.raises(ValueError, match="no usable HIP device"):
            rr.StreamToPdu(0.5, 10, 0)
