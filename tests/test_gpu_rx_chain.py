"""GPU: the receive chain DESIGN 4.17 names, rr.FmMulti -> rr.SymbolSync -> rr.HdlcReceiver, with no host read before the frames,
against the Python machines of tests/rx_chain_helpers.py (symsync_model.SymbolSync -> hdlcrx_helpers.ModelReceiver).  Every
comparison is bit for bit: frames (position, bytes, repaired flag), the three counters, the symbols consumed; there is no tolerance
in this file.  The conditions that keep the equalities from being vacuous — counts that differ from stream to stream in every
push, frames across every push boundary, repaired frames, every packet recovered — are asserted on the models by
tests/test_rx_chain_cpu.py; the models' answers are computed once per signal and shared."""
import numpy as np
import pytest
import torch

import rustradio_amd as rr
import rx_chain_helpers as rc

pytestmark = pytest.mark.gpu


def stream0():
    return torch.cuda.current_stream().cuda_stream


def snapshot(rx):
    return rx.result(), [tuple(int(v) for v in r) for r in rx.stats()], [int(v) for v in rx.consumed()]


def wanted(push):
    return push["frames"], push["stats"], push["consumed"]


# ---- 1., 2. SymbolSync -> HdlcReceiver on the counts SymbolSync left on the device --------------------------------------------------
@pytest.mark.parametrize("flags", [0, rr.HDLC_FIX_BITS], ids=["plain", "fix-bits"])
@pytest.mark.parametrize("lanes", [1, 64])
def test_symbol_sync_hands_its_own_ragged_counts_to_the_receiver(lanes, flags):
    """66 streams whose counts differ in every push (a second, partly filled wave under the 64-lane mapping), three pushes on one
    HIP stream, counts_dev() passed straight to push_dev.  fix-bits: the copy of the signal with one wrong bit inside a frame of
    three streams, repaired there and nowhere else."""
    assert rc.FIX == rr.HDLC_FIX_BITS
    x = rc.ragged_samples(bool(flags))
    N, n = x.shape
    model = rc.ragged_model(flags)
    with rr.build_options(sync_lanes=lanes):
        ss = rr.SymbolSync(*rc.RAGGED_PRM, nstreams=N)
    assert ss.streams_per_wave == lanes
    rx = rr.HdlcReceiver(N, 1, rc.RAGGED_MAX_SIZE, nrzi=True, descrambler=rc.G3RUH, flags=flags)
    dx = torch.from_numpy(x.copy()).cuda()
    s, at, produced = stream0(), 0, np.zeros(N, np.int64)
    for k, want in zip(rc.ragged_cuts(n), model):
        win = dx[:, at:at + k].contiguous()
        syms = torch.zeros((N, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ss.push_dev(win.data_ptr(), k, k, syms.data_ptr(), None, k, s)
        rx.push_dev(syms.data_ptr(), k, k, ss.counts_dev(), s)                  # nothing read by the host in between
        got = snapshot(rx)                                                      # (waits for both)
        assert got == wanted(want), (k, lanes)
        counts = ss.produced()
        assert [int(v) for v in counts] == want["counts"]
        produced += counts.astype(np.int64)
        assert got[2] == produced.tolist()                                      # consumed(): the running sum of produced()
        at += k
    assert at == n
    fixed = [st[2] for st in got[1]]
    if flags:
        assert [c for c in range(N) if fixed[c]] == list(rc.FLIPPED_ROWS) and all(fixed[c] == 1 for c in rc.FLIPPED_ROWS)
    else:
        assert not any(fixed)


# ---- 3., 4. FmMulti -> SymbolSync -> HdlcReceiver ------------------------------------------------------------------------------------
def run_fm_chain(host_twin):
    """the band in three work_dev calls of unequal size (the second leaves fewer than 64 demodulated samples per channel), each
    followed by the two pushes on the same HIP stream: out_cap is SymbolSync's in_stride, `produced` its n and the receiver's n_cap
    -> per call (produced, the windows FmMulti wrote [5, produced], snapshot of the receiver)"""
    x = rc.fm_samples()
    C, n = rc.FM_NCHAN, len(x)
    out_cap = n // rc.FM_DECI + 64
    fm = rr.FmMulti(rc.fm_taps(), 1, rc.FM_DECI, 1.0)
    ss = rr.SymbolSync(*rc.FM_PRM, nstreams=C)
    rx = rr.HdlcReceiver(C, 1, rc.FM_MAX_SIZE, **rc.FM_RX_KW)
    dx = torch.from_numpy(x.view(np.float32).copy()).cuda()
    dy = torch.full((C * out_cap,), -7777.25, dtype=torch.float32, device="cuda")
    dsyms = torch.zeros((C, out_cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s, pos, calls = stream0(), 0, []
    for size in (n // 3 + 11, 450, n):
        in_len = min(size, n - pos)
        st, c, p, need = fm.work_dev(dx.data_ptr() + 8 * pos, in_len, dy.data_ptr(), out_cap, s)
        assert p <= out_cap
        pos += c
        ss.push_dev(dy.data_ptr(), out_cap, p, dsyms.data_ptr(), None, out_cap, s)
        if host_twin:
            counts = [int(v) for v in ss.produced()]
            rx.push(dsyms.cpu().numpy()[:, :p], counts)
        else:
            rx.push_dev(dsyms.data_ptr(), out_cap, p, ss.counts_dev(), s)       # nothing read by the host before the frames
        snap = snapshot(rx)
        # (the windows are read after the frames; nothing has written them since)
        calls.append((p, dy.cpu().numpy().reshape(C, out_cap)[:, :p].copy(), snap))
    assert pos > n - 1024 and len(calls) == 3                                   # (all but a partial block of the filter at most)
    return calls


@pytest.fixture(scope="module")
def fm_chain():
    return run_fm_chain(False)


def test_fm_multi_to_frames_plumbing(fm_chain):
    """the windows FmMulti wrote (channel c at out + c out_cap, `produced` samples each), downloaded and run through the two models
    on the host: frames, counters and consumed counts of the device chain equal the models' exactly — the models read the
    device's own front-end output, so no tolerance enters"""
    ps = [p for p, _, _ in fm_chain]
    assert len(set(ps)) == 3 and 0 < ps[1] < 64 and min(ps[0], ps[2]) > 2000, ps
    rows = np.concatenate([w for _, w, _ in fm_chain], axis=1)
    assert np.isfinite(rows).all() and not (rows == np.float32(-7777.25)).any()
    model = rc.fm_model(rows, ps)
    for (p, _, snap), want in zip(fm_chain, model):
        assert snap == wanted(want), p
    assert sum(len(f) for push in model for f in push["frames"]) == 15


def test_fm_multi_to_frames_end_to_end(fm_chain):
    """every channel delivers the packets that were modulated onto its station, in order, nothing repaired"""
    for ch in range(rc.FM_NCHAN):
        frames = [f for _, _, snap in fm_chain for f in snap[0][ch]]
        assert [f[1] for f in frames] == rc.fm_payloads(ch) and not any(f[2] for f in frames), ch
    assert fm_chain[-1][2][1] == [(3, 0, 0)] * rc.FM_NCHAN


def test_fm_multi_to_frames_host_twin(fm_chain):
    """the same chain with the symbols and counts downloaded and fed to the receiver's host path: the same frames, counters and
    consumed counts, call for call"""
    twin = run_fm_chain(True)
    assert [(p, snap) for p, _, snap in twin] == [(p, snap) for p, _, snap in fm_chain]
    for (_, a, _), (_, b, _) in zip(twin, fm_chain):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
