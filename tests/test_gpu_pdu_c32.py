"""GPU: rr_stream_to_pdu_c32 (StreamToPdu<Complex>: kernels_pdu.hip k_pdu_count<true> in front of the shared closed form) against
tests/pdu_model.py StreamToPduSeq, push by push and byte for byte, on the edge and seam geometry of tests/test_gpu_pdu.py; the
type refusals; and the f32 handle filing the same bursts."""
import numpy as np
import pytest
import torch

import pdu_model as pm
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
F32 = np.float32
T = 2048                    # PDU_T (samples of a tile): kernels.hpp


def labelled_c32(n, seed=0):
    """n distinct Complex samples, every seventh one a NaN with its own payload bits: a PDU with the wrong samples, or one whose
    bits went through arithmetic, cannot pass for the right one"""
    x = np.empty(n, np.complex64)
    u = x.view(np.uint32).reshape(n, 2)
    u[:, 0] = np.arange(n, dtype=np.uint32) + np.uint32(0x3F000000 + 977 * seed)
    u[:, 1] = np.uint32(0xBF000000) + 3 * np.arange(n, dtype=np.uint32)
    u[::7, 0] = np.uint32(0x7F900000) + np.arange(0, n, 7, dtype=np.uint32)       # signalling NaNs
    return x


def trigger_of(n, bursts):
    t = np.zeros(n, F32)
    for r, length in bursts:
        t[r:r + length] = 1.0
    return t


def want_of(n, trig, thr, max_size, tail, splits):
    """the model over sample LABELS (the positions) -> per push [(first, [positions])]"""
    return pm.stream_to_pdu_seq(list(range(n)), trig, thr, max_size, tail, list(splits))


def push_all(b, x, trig, splits, dev=False):
    cuts = [0] + sorted(splits) + [len(x)]
    per = []
    for a, c in zip(cuts[:-1], cuts[1:]):
        if dev and c > a:
            d_x = torch.from_numpy(x[a:c].view(F32).copy()).cuda()
            d_t = torch.from_numpy(trig[a:c].copy()).cuda()
            b.push_dev(d_x.data_ptr(), d_t.data_ptr(), c - a)
            rec = b.records()
        else:
            rec = b.push(x[a:c], trig[a:c])
        p, n_total = b.arena_dev()
        assert (n_total == 0 and p is None and len(rec) == 0) if c == a else (n_total == b.max_size + (c - a) and p)
        end = 0
        for r in rec:
            assert int(r["start"]) >= end and int(r["start"]) + int(r["len"]) <= n_total and r["ok"] == 1
            assert r["mean"] == 0 and r["mid"] == 0
            end = int(r["start"]) + int(r["len"])
        per.append([(int(r["stream_pos"]), b.pdu(i, rec)) for i, r in enumerate(rec)])
    return per


def check_stream(x, trig, thr, max_size, tail, splits=(), dev=False):
    want = want_of(len(x), trig, thr, max_size, tail, splits)
    b = rr.StreamToPduC32(thr, max_size, tail)
    b.max_size = max_size
    got = push_all(b, x, trig, splits, dev)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert [f for f, _ in g] == [f for f, _ in w], (k, [(f, len(p)) for f, p in g], [(f, len(p)) for f, p in w])
        for (f, gp), (_, wp) in zip(g, w):
            assert gp.dtype == np.complex64 and gp.tobytes() == x[np.array(wp, np.int64)].tobytes(), (k, f)
    return b, want


def test_a_burst_across_three_pushes():
    n = 400
    trig = trigger_of(n, [(50, 200)])
    for splits in ([100, 200], [100, 200, 251, 252, 260, 300]):
        b, want = check_stream(labelled_c32(n), trig, 0.5, 300, 3 if len(splits) == 2 else 60, splits)
        assert sum(len(w) for w in want) == 1
    check_stream(labelled_c32(n), trig, 0.5, 300, 3, [100, 200], dev=True)


def test_a_burst_that_outgrows_max_size_and_tail_0():
    n = 300
    b, want = check_stream(labelled_c32(n), trigger_of(n, [(20, 50), (80, 4)]), 0.5, 30, 0)
    assert [[len(p) for _, p in w] for w in want] == [[4]]
    b, want = check_stream(labelled_c32(n), trigger_of(n, [(20, 28), (50, 4), (60, 4)]), 0.5, 30, 5, [40])
    assert sum(len(w) for w in want) == 1
    for L, tail, max_size, npdus in [(40, 0, 40, 1), (41, 0, 40, 0), (30, 10, 39, 0), (1, 0, 1, 1), (5, 0, 0, 0)]:
        for splits in ([], [60], [75]):
            b, want = check_stream(labelled_c32(n), trigger_of(n, [(50, L)]), 0.5, max_size, tail, splits)
            assert sum(len(w) for w in want) == npdus


@pytest.mark.parametrize("splits", [[], [T], [T - 1, T + 1]])
def test_edges_on_the_last_sample_of_a_tile_and_the_first_of_the_next(splits):
    n = 3 * T + 1
    bursts = [(T - 1, 10), (2 * T - 8, 8), (2 * T + 40, 5), (3 * T - 1, 1)]      # rises at T - 1; falls at 2 T; rises at 3 T - 1, falls at 3 T
    trig = trigger_of(n, bursts)
    b, want = check_stream(labelled_c32(n), trig, 0.5, 64, 1, splits)
    assert sum(len(w) for w in want) == 4
    if not splits:
        pos, val = b.edges()
        assert list(pos) == [T - 1, T + 9, 2 * T - 8, 2 * T, 2 * T + 40, 2 * T + 45, 3 * T - 1, 3 * T]


def test_pushes_of_one_sample():
    n = 90
    trig = trigger_of(n, [(10, 20), (50, 3)])
    b, want = check_stream(labelled_c32(n), trig, 0.5, 40, 4, list(range(1, n)))
    assert sum(len(w) for w in want) == 2
    check_stream(labelled_c32(n), trig, 0.5, 40, 4, [30, 31])          # ... and one between two long pushes, on the tail's end


def test_the_type_refusals():
    f32, c32 = rr.StreamToPdu(0.5, 16, 0), rr.StreamToPduC32(0.5, 16, 0)
    trig = trigger_of(32, [(4, 8)])
    assert len(f32.push(np.arange(32, dtype=F32), trig)) == 1 and len(c32.push(labelled_c32(32), trig)) == 1
    out = np.zeros(64, np.complex64)
    L = rr.lib()
    assert L.rr_pdu_fetch(c32._h, 0, out.ctypes.data, 8) != 0 and "the PDUs are not f32" in rr.last_error()
    assert L.rr_pdu_fetch_c32(f32._h, 0, out.ctypes.data, 8) != 0 and "the PDUs are not Complex" in rr.last_error()
    assert L.rr_stream_to_pdu_push_c32(f32._h, out.ctypes.data, trig.ctypes.data, 8) != 0 and "the PDUs are not Complex" in rr.last_error()
    assert L.rr_stream_to_pdu_push(c32._h, out.ctypes.data, trig.ctypes.data, 8) != 0 and "the PDUs are not f32" in rr.last_error()
    w = rr.Wpcr()
    d_syms = torch.zeros(128, dtype=torch.float32, device="cuda")
    assert L.rr_wpcr_process_pdus(w._h, c32._h, d_syms.data_ptr(), None) != 0 and rr.last_error() == "wpcr: the PDUs are not f32"
    assert L.rr_wpcr_process_pdus(w._h, f32._h, d_syms.data_ptr(), None) == 0
    # nothing of the refused calls was done: both handles still hold their one PDU
    assert len(f32.records()) == 1 and len(c32.records()) == 1
    with pytest.raises(RuntimeError, match="forms PDUs"):
        c32.work(np.zeros(4, np.complex64), 4)
    with pytest.raises(ValueError, match="max_size beyond 512000 samples"):
        rr.StreamToPduC32(0.5, 512_001, 0)


def test_an_f32_handle_files_the_same_bursts():
    rng = np.random.default_rng(5)
    n = 2 * T + 300
    trig = np.repeat(rng.random(n // 40 + 1) < 0.5, 40)[:n].astype(F32)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    splits = [T - 3, T + 900]
    f32, c32 = rr.StreamToPdu(0.5, 200, 7), rr.StreamToPduC32(0.5, 200, 7)
    cuts = [0] + splits + [n]
    total = 0
    for a, c in zip(cuts[:-1], cuts[1:]):
        rf, rc = f32.push(np.ascontiguousarray(x.real[a:c]), trig[a:c]), c32.push(x[a:c], trig[a:c])
        assert [(int(r["stream_pos"]), int(r["len"])) for r in rf] == [(int(r["stream_pos"]), int(r["len"])) for r in rc]
        for i in range(len(rc)):
            assert np.array_equal(c32.pdu(i, rc).real.view(np.uint32), f32.pdu(i, rf).view(np.uint32))
        (p0, v0), (p1, v1) = f32.edges(), c32.edges()
        assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
        total += len(rc)
    assert total > 10
