"""GPU: rr_burst_saver (examples/burst_saver.rs behind one handle) held to its definition.

The yardstick (`hold`): for every push the saver's edges are rr_burst_edges of an rr_burst_detector given the same pushes, and
its records and payload bytes are those of tests/pdu_model.py StreamToPduSeq fed tests/saver_model.py DelaySeq's output and
those edges — bit for bit, per push.  The model moves sample LABELS (input position + 1, 0 for Delay's zeros), so a payload that
went through arithmetic, or came from the wrong place, cannot pass.  A second yardstick takes the edges from the reference's own
f32 fold instead (burst_model.iir_ref_f32), on inputs whose envelope keeps a proven distance from the threshold."""
import os
import re

import numpy as np
import pytest
import torch

import burst_model as bm
import pdu_model as pm
import rustradio_amd as rr
import saver_model as sm

pytestmark = pytest.mark.gpu
F32 = np.float32
T = 2048                    # IIR_T = PDU_T: kernels.hpp


def cuts_every(n, push):
    return list(range(push, n, push))


def payload_of(x, labels):
    lab = np.asarray(labels, np.int64)
    out = np.zeros(len(lab), np.complex64)
    out[lab > 0] = x[lab[lab > 0] - 1]
    return out.tobytes()


def hold(x, splits, alpha, thr, delay, max_size, tail, ref_edges=False, b=None):
    """-> (the saver, [(stream_pos, payload bytes)] of the whole stream, PDUs per push, all edges absolute)"""
    x = np.ascontiguousarray(x, np.complex64)
    b = rr.BurstSaver(alpha, thr, delay, max_size, tail) if b is None else b
    det = rr.BurstDetector(alpha, thr)
    ref = sm.SaverSeq(alpha, thr, 0, 0, 0)
    dl, seq = sm.DelaySeq(delay), pm.StreamToPduSeq(max_size, tail)
    cuts = [0] + sorted(splits) + [len(x)]
    pdus, per, edges = [], [], []
    for a, c in zip(cuts[:-1], cuts[1:]):
        rec = b.push(x[a:c])
        pos, val = b.edges()
        if c > a:
            st, cons, prod, need, env = det.work(x[a:c], c - a)
            assert prod == c - a
            dpos, dval = det.edges()
        else:
            dpos, dval = np.zeros(0, np.uint64), np.zeros(0, bool)
        assert np.array_equal(pos, dpos) and np.array_equal(val, dval), (a, c)
        tags = [(int(p), bool(v)) for p, v in zip(pos, val)]
        if ref_edges:
            tags = ref.push(x[a:c])[1]
            assert tags == [(int(p), bool(v)) for p, v in zip(pos, val)], (a, c)
        dl.src += list(range(a + 1, c + 1))
        want = seq.work(dl.work(c - a)[4], tags)
        p, n_total = b.arena_dev()
        assert (n_total == 0 and p is None and len(rec) == 0) if c == a else (n_total == max_size + (c - a) and p)
        assert [int(r["stream_pos"]) for r in rec] == [f for f, _ in want], (a, c, rec, [(f, len(q)) for f, q in want])
        end = 0
        for i, (r, (f, labels)) in enumerate(zip(rec, want)):
            assert int(r["start"]) >= end and int(r["start"]) + int(r["len"]) <= n_total
            assert r["ok"] == 1 and r["mean"] == 0 and r["mid"] == 0 and int(r["len"]) == len(labels)
            end = int(r["start"]) + int(r["len"])
            got = b.pdu(i, rec).tobytes()
            assert got == payload_of(x, labels), (a, c, f)
            pdus.append((f, got))
        per.append(len(rec))
        edges += [(a + p, v) for p, v in tags]
    return b, pdus, per, edges


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("push", [4096, 2049])
@pytest.mark.parametrize("delay", [0, 1, 3000, 5000])
def test_definition_over_delays_and_pushes(delay, push):
    n = 20000
    x = bm.burst_signal(n, 100 + delay)
    b, pdus, per, edges = hold(x, cuts_every(n, push), 0.1, 0.004, delay, 6000, 100)
    assert len(pdus) == 3 and len(edges) >= 6                     # (alpha 0.1: the 3-sample burst never lifts the envelope that far)


def test_a_run_of_pushes_shorter_than_the_delay():
    """delay 3000 in pushes of 100: thirty pushes in which no input sample reaches the arena, then fifty more"""
    n = 8000
    x = bm.burst_signal(n, 7)
    b, pdus, per, edges = hold(x, cuts_every(n, 100), 0.1, 0.004, 3000, 2500, 40)
    assert len(per) == 80 and len(pdus) == 3
    first = pdus[0][1]                                             # the burst at 666 .. 1599: all of it Delay's zeros
    assert pdus[0][0] < 3000 and first == bytes(len(first))
    assert any(np.frombuffer(p, np.complex64).any() for _, p in pdus[1:])


def test_a_burst_that_rises_in_one_push_and_whose_tail_ends_two_pushes_later():
    n = 2600
    x = (0.003 * np.exp(1j * np.arange(n))).astype(np.complex64)
    x[1000:1500] += 0.1
    b, pdus, per, edges = hold(x, [1200, 1550], 0.1, 0.004, 300, 1000, 100)
    assert per == [0, 0, 1] and len(edges) == 2 and edges[0][0] < 1200 <= edges[1][0] < 1550 <= edges[1][0] + 100


def test_a_burst_in_the_first_delay_positions_starts_with_zeros():
    n = 3000
    x = (0.003 * np.exp(1j * np.arange(n))).astype(np.complex64)
    x[100:600] += 0.1
    b, pdus, per, edges = hold(x, [1024], 0.1, 0.004, 300, 1000, 50)
    (f, p), = pdus
    v = np.frombuffer(p, np.complex64)
    assert 100 < f < 300 and not v[:300 - f].any() and v[300 - f:].all()


def test_max_size_exceeded_and_tail_0():
    n = 20000
    x = bm.burst_signal(n, 3)
    b, pdus, per, edges = hold(x, cuts_every(n, 4096), 0.1, 0.004, 3000, 3500, 0)       # the burst of 4000 is dropped
    assert len(pdus) == 2
    b, pdus, per, edges = hold(x, cuts_every(n, 2049), 0.1, 0.004, 1, 2400, 0)          # ... and the one of 3000
    assert len(pdus) == 1 and all(len(p) // 8 <= 2400 for _, p in pdus)
    b, pdus, per, edges = hold(x, [], 0.1, 0.004, 0, 0, 0)
    assert pdus == []


# ---- 2. against the reference's f32 chain -----------------------------------------------------------------------------------------------
REF_CASES = [(seed, alpha, delay, push) for seed, alpha in [(1, 0.1), (2, 0.5), (3, 0.05), (4, 0.1), (5, 0.5), (6, 0.05)]
             for delay, push in [(0, 4096), (3000, 2049)]]


def margin(x, alpha, thr, calls):
    """-> the least |truth - threshold| - (the GPU's bound + the reference's bound) over the stream, float64"""
    m2 = bm.mag2_f32(x)
    t, _ = bm.iir_truth(m2, alpha)
    allow = bm.bound_gpu_any(t, m2, alpha, calls) + bm.bound_ref(float(np.max(m2)), alpha)
    return float(np.min(np.abs(t - float(F32(thr))) - allow))


def test_ref_cases_are_twelve():
    assert len(REF_CASES) >= 12


@pytest.mark.parametrize("seed,alpha,delay,push", REF_CASES)
def test_against_the_references_f32_chain(seed, alpha, delay, push):
    n = 12000
    x = bm.burst_signal(n, seed)
    splits = cuts_every(n, push)
    assert margin(x, alpha, 0.004, len(splits) + 1) > 0.0          # asserted, never skipped: the seeds were chosen on the CPU
    b, pdus, per, edges = hold(x, splits, alpha, 0.004, delay, 4000, 100, ref_edges=True)
    assert len(pdus) >= 3


# ---- 3. the envelope ----------------------------------------------------------------------------------------------------------------------
def test_the_envelope_is_the_detectors_and_optional():
    n = 3 * T + 77
    x = bm.burst_signal(n, 9)
    a, b2, det = rr.BurstSaver(0.1, 0.004, 700, 3000, 20), rr.BurstSaver(0.1, 0.004, 700, 3000, 20), rr.BurstDetector(0.1, 0.004)
    d_x = torch.from_numpy(x.view(F32).copy()).cuda()
    for lo, hi in [(0, T), (T, T + 1), (T + 1, n)]:
        rec, env = a.push(x[lo:hi], env=True)
        st, c, p, need, want = det.work(x[lo:hi], hi - lo)
        assert np.array_equal(env.view(np.uint32), want.view(np.uint32))
        # the device call, with no envelope asked for
        b2.push_dev(d_x.data_ptr() + 8 * lo, hi - lo)
        rec2 = b2.records()
        assert rec.tobytes() == rec2.tobytes()
        assert all(a.pdu(i, rec).tobytes() == b2.pdu(i, rec2).tobytes() for i in range(len(rec)))
        assert all(np.array_equal(u, v) for u, v in zip(a.edges(), b2.edges()))
    d_env = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    c3, det3 = rr.BurstSaver(0.1, 0.004, 700, 3000, 20), rr.BurstDetector(0.1, 0.004)
    c3.push_dev(d_x.data_ptr(), n, d_env.data_ptr())
    c3.sync()
    want = det3.work(x, n)[4]
    assert np.array_equal(d_env.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 4. independence of the split ---------------------------------------------------------------------------------------------------------
def test_one_push_and_seven_file_the_same_pdus():
    n, met = 14000, 0
    for seed in (21, 22, 23):
        x = bm.burst_signal(n, seed)
        one = hold(x, [], 0.1, 0.004, 900, 3000, 60)
        seven = hold(x, cuts_every(n, 2000), 0.1, 0.004, 900, 3000, 60)
        if one[3] == seven[3]:                                      # the two detector runs agree on every edge
            met += 1
            assert one[1] == seven[1] and len(one[1]) >= 2
    assert met >= 1


# ---- 5. the launch count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, T, T + 1, 5000])
def test_launches_depend_on_n_alone(n):
    zero = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    busy = np.zeros(n, np.complex64)
    busy[(np.arange(n) // 1) % 2 == 0] = 1.0                        # alpha 1: the envelope is the power itself, an edge at every sample
    d_busy = torch.from_numpy(busy.view(F32).copy()).cuda()
    torch.cuda.synchronize()
    counts = []
    for d in (zero, d_busy):
        b = rr.BurstSaver(1.0, 0.5, 5, 40, 1)
        l0 = int(rr.lib().rr_debug_kernel_launches())
        b.push_dev(d.data_ptr(), n)
        counts.append(int(rr.lib().rr_debug_kernel_launches()) - l0)
        nedges = len(b.edges()[0])
        assert nedges == (0 if d is zero else n)
    tile, launches = b.dims(n)
    assert tile == T and counts == [launches, launches]
    assert launches == (1 if n <= T else 3) + 1 + 5 + int(np.ceil(np.log2(n // 2 + 1)))


def test_an_empty_push_launches_nothing_and_forgets_nothing():
    n = 2600
    x = (0.003 * np.exp(1j * np.arange(n))).astype(np.complex64)
    x[1000:1500] += 0.1
    b, pdus, per, edges = hold(x, [1200, 1200, 1200], 0.1, 0.004, 300, 1000, 100)
    assert per == [0, 0, 0, 1]
    b = rr.BurstSaver(0.1, 0.004, 300, 1000, 100)
    assert len(b.push(x)) == 1 and b.dims(0) == (T, 0)
    l0 = int(rr.lib().rr_debug_kernel_launches())
    b.push_dev(0, 0)
    assert int(rr.lib().rr_debug_kernel_launches()) == l0
    assert len(b.records()) == 0 and b.arena_dev() == (None, 0) and len(b.edges()[0]) == 0


# ---- 6. a NaN in the middle of a burst ----------------------------------------------------------------------------------------------------
def test_a_nan_sample_ends_the_edges_and_keeps_its_bits():
    n = 20000
    x = bm.burst_signal(n, 5)
    clean = hold(x, cuts_every(n, 4096), 0.1, 0.004, 50, 6000, 100)
    k = 12000                                                      # inside the burst at 10000 .. 14000
    y = x.copy()
    y.view(np.uint32)[2 * k] = 0x7FC12345
    b = rr.BurstSaver(0.1, 0.004, 50, 6000, 100)
    got = hold(y, cuts_every(n, 4096), 0.1, 0.004, 50, 6000, 100, b=b)
    rec, env = rr.BurstSaver(0.1, 0.004, 50, 6000, 100).push(y, env=True)
    assert not np.isnan(env[:k]).any() and np.isnan(env[k:]).all()
    assert got[3][-1] == (k, False) and got[3][:-1] == [e for e in clean[3] if e[0] < k]
    assert got[1][0] == clean[1][0]                                # the PDU filed before it
    f, p = got[1][-1]
    v = np.frombuffer(p, np.uint32)
    assert f + len(p) // 8 == k + 100 and v[2 * (k + 50 - f)] == 0x7FC12345


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_no_launch():
    L = rr.lib()
    b, other = rr.BurstSaver(0.1, 0.004, 10, 100, 5), rr.StreamToPduC32(0.5, 8, 0)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    l0 = int(L.rr_debug_kernel_launches())
    for args, msg in [((2.0, 0.5, 1, 1, 1), "alpha out of range"), ((float("nan"), 0.5, 1, 1, 1), "alpha out of range"),
                      ((0.5, 0.5, 1, 512_001, 1), "max_size beyond 512000 samples"),
                      ((0.5, 0.5, 1_024_001, 1, 1), "delay: more than 1,024,000 samples")]:
        assert not L.rr_burst_saver_create(*args) and rr.last_error() == msg
    with pytest.raises(RuntimeError, match="window longer than 1024000 samples"):
        b.push_dev(d.data_ptr(), 1_024_001)
    with pytest.raises(RuntimeError, match="null argument"):
        b.push_dev(0, 4)
    assert L.rr_burst_saver_push(b._h, None, 4, None) != 0 and "null argument" in rr.last_error()
    with pytest.raises(RuntimeError, match="forms PDUs"):
        b.work(np.zeros(4, np.complex64), 4)
    out = np.zeros(8, F32)
    assert L.rr_pdu_fetch(b._h, 0, out.ctypes.data, 1) != 0 and "the PDUs are not f32" in rr.last_error()
    assert L.rr_stream_to_pdu_push_c32(b._h, out.ctypes.data, out.ctypes.data, 1) != 0
    assert L.rr_stream_to_pdu_push_dev(b._h, d.data_ptr(), d.data_ptr(), 4, None) != 0 and "burst saver" in rr.last_error()
    assert L.rr_burst_saver_push_dev(other._h, d.data_ptr(), 4, None, None) != 0
    assert "not a burst saver handle" in rr.last_error()
    assert int(L.rr_debug_kernel_launches()) == l0


# ---- 8. PduWriter -------------------------------------------------------------------------------------------------------------------------
def test_save_is_pdu_writer(tmp_path):
    n = 20000
    x = bm.burst_signal(n, 4)
    b = rr.BurstSaver(0.1, 0.004, 3000, 6000, 100)
    rec = b.push(x[:16000])
    paths = b.save(tmp_path)
    assert len(paths) == len(rec) == 2
    rec2 = b.push(x[16000:])
    paths += b.save(tmp_path)
    assert len(rec2) == 1 and sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in paths)
    names = [os.path.basename(p) for p in paths]
    assert all(re.fullmatch(r"\d+-\d+", nm) for nm in names)
    assert [int(nm.split("-")[1]) for nm in names] == [0, 1, 2]
    assert [int(nm.split("-")[0]) for nm in names] == sorted(int(nm.split("-")[0]) for nm in names)
    assert open(paths[2], "rb").read() == b.pdu(0, rec2).astype("<c8").tobytes()
    assert all(os.path.getsize(p) == 8 * int(r["len"]) for p, r in zip(paths[:2], rec))


# ---- 9. fuzz ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(3))
def test_fuzz(block):
    rng = np.random.default_rng(1000 + block)
    filed = 0
    for it in range(10):
        n = int(rng.integers(1, 20001))
        alpha = float(rng.choice([0.01, 0.1, 0.5]))
        delay, tail, max_size = int(rng.integers(0, 6001)), int(rng.integers(0, 3001)), int(rng.integers(0, 8001))
        splits = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 6))))
        x = bm.burst_signal(n, 5000 + 10 * block + it)
        b, pdus, per, edges = hold(x, splits, alpha, 0.004, delay, max_size, tail)
        filed += len(pdus)
    assert filed > 0
