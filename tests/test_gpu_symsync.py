"""GPU: rr_symbol_sync (kernels_sync.hip) against the reference's sequential machine of tests/symsync_model.py.  Every comparison is
bit for bit — the uint32 views of symbols and clock values, equal counts, equal state; there is no tolerance anywhere in this file.

The model's answers are computed once per signal (functools.lru_cache) and shared by the tests that need them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rustradio_amd as rr
import symsync_model as sm
from symsync_dev import SENTINEL, _DevMem, dev_push, u32

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def signal_9600():
    """about 21,000 samples: 4000 noisy symbols with a +0.3 % clock offset"""
    x = sm.nrz(4000, sm.AX25_9600[0], 1, offset=0.003, smooth=3, noise=0.15)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model_whole(prm_key):
    prm = {"9600": sm.AX25_9600, "adaptive": sm.ADAPTIVE_9600}[prm_key]
    m = sm.SymbolSync(*prm)
    syms, clk, idx = m.run(signal_9600())
    return syms, clk, idx, m.state(), m.clock_updates


# ---- 1. the reference's own test ------------------------------------------------------------------------------------------------------
def test_reference_own_test_through_both_entry_points():
    """symbol_sync.rs:229-242: 10 zeros, sps 4, max_deviation 1, taps [1.0] -> 2 symbols"""
    h = rr.SymbolSync(4.0, 1.0, [1.0])
    syms, clk = h.push(np.zeros(10, np.float32))
    assert len(syms[0]) == 2 and clk[0].tolist() == [4.0, 4.0] and h.produced().tolist() == [2]
    h = rr.SymbolSync(4.0, 1.0, [1.0])
    counts, syms, clk = dev_push(h, np.zeros(10, np.float32))
    assert counts.tolist() == [2] and u32(syms[0]).tolist() == [0, 0] and clk[0].tolist() == [4.0, 4.0]
    with pytest.raises(RuntimeError, match="SymbolSync runs nstreams streams"):
        h.work(np.zeros(4, np.float32), 4)


# ---- 2., 3. one stream in one push ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["9600", "adaptive"])
def test_one_stream_one_push(key):
    """ax25-9600-rx's parameters, and the adaptive taps [0.1, 0.9] with max_deviation 0.5 — about 2000 clock updates, each with a
    rounding of its own: the case a contracted multiply-add in the filter or in `+ sps` cannot pass"""
    prm = {"9600": sm.AX25_9600, "adaptive": sm.ADAPTIVE_9600}[key]
    syms, clk, idx, state, updates = model_whole(key)
    assert 20000 < len(signal_9600()) < 22000 and abs(len(syms) - 4000) <= 2 and updates > 1500
    if key == "adaptive":
        assert len(set(u32(clk).tolist())) > 1000
    h = rr.SymbolSync(*prm)
    counts, s, c = dev_push(h, signal_9600())
    assert counts.tolist() == [len(syms)]
    assert np.array_equal(u32(s[0]), u32(syms)) and np.array_equal(u32(c[0]), u32(clk))
    assert sm.states_equal(h.state(0), state)


# ---- 4. carried state ----------------------------------------------------------------------------------------------------------------
def test_any_split_into_pushes_is_the_one_push():
    x = signal_9600()[:6000]
    whole = sm.SymbolSync(*sm.ADAPTIVE_9600)
    want_s, want_c, _ = whole.run(x)
    m = sm.SymbolSync(*sm.ADAPTIVE_9600)
    h = rr.SymbolSync(*sm.ADAPTIVE_9600)
    got_s, got_c, pos = [], [], 0
    for ln in (1, 63, 64, 65, 0, 777, len(x) - 970):
        ms, mc, _ = m.run(x[pos:pos + ln])
        counts, s, c = dev_push(h, x[pos:pos + ln])
        assert counts.tolist() == [len(ms)] and np.array_equal(u32(s[0]), u32(ms)) and np.array_equal(u32(c[0]), u32(mc)), ln
        assert sm.states_equal(h.state(0), m.state()), ln
        got_s.append(s[0]); got_c.append(c[0])
        pos += ln
    assert pos == len(x)
    assert np.array_equal(u32(np.concatenate(got_s)), u32(want_s)) and np.array_equal(u32(np.concatenate(got_c)), u32(want_c))


def test_two_handles_on_two_hip_streams_do_not_disturb_each_other():
    xa, xb = signal_9600()[:4000], signal_9600()[7000:11000]
    want = [sm.SymbolSync(*sm.ADAPTIVE_9600).run(xa), sm.SymbolSync(*sm.AX25_9600).run(xb)]
    ha, hb = rr.SymbolSync(*sm.ADAPTIVE_9600), rr.SymbolSync(*sm.AX25_9600)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    cuts = (0, 500, 1100, 1101, 2500, 4000)
    d_a, d_b = torch.from_numpy(xa.copy()).cuda(), torch.from_numpy(xb.copy()).cuda()
    outs = {k: [torch.zeros(4000, dtype=torch.float32, device="cuda") for _ in range(len(cuts) - 1)] for k in ("as", "ac", "bs", "bc")}
    torch.cuda.synchronize()
    counts = {"a": [], "b": []}
    for i in range(len(cuts) - 1):                          # every push is enqueued before anything is waited for
        lo, n = cuts[i], cuts[i + 1] - cuts[i]
        ha.push_dev(d_a.data_ptr() + 4 * lo, n, n, outs["as"][i].data_ptr(), outs["ac"][i].data_ptr(), 4000, sa.cuda_stream)
        hb.push_dev(d_b.data_ptr() + 4 * lo, n, n, outs["bs"][i].data_ptr(), outs["bc"][i].data_ptr(), 4000, sb.cuda_stream)
        # (the counts of a push are valid until the handle's next push: read them now, on the push's own stream)
        with torch.cuda.stream(sa):
            ca = torch.as_tensor(_DevMem(ha.counts_dev(), 8), device="cuda").clone()
        with torch.cuda.stream(sb):
            cb = torch.as_tensor(_DevMem(hb.counts_dev(), 8), device="cuda").clone()
        counts["a"].append(ca); counts["b"].append(cb)
    torch.cuda.synchronize()
    for k, w in (("a", want[0]), ("b", want[1])):
        ks = [int(np.frombuffer(t.cpu().numpy().tobytes(), np.uint64)[0]) for t in counts[k]]
        s = np.concatenate([outs[k + "s"][i][:ks[i]].cpu().numpy() for i in range(len(ks))])
        c = np.concatenate([outs[k + "c"][i][:ks[i]].cpu().numpy() for i in range(len(ks))])
        assert np.array_equal(u32(s), u32(w[0])) and np.array_equal(u32(c), u32(w[1])), k


# ---- 5. many streams, both stream-to-lane mappings ------------------------------------------------------------------------------------
N_MULTI = 5003


@functools.lru_cache(maxsize=None)
def row(c):
    """row c of every multi-stream test: its own seed and clock offset; row 1 all zeros, row 2 with NaN / +-Inf / -0.0 sprinkled
    in, row 3 with the idle gap -> (samples, the model run alone: symbols, clock values, state)"""
    sps = sm.ADAPTIVE_9600[0]
    if c == 1:
        x = np.zeros(N_MULTI, np.float32)
    else:
        x = sm.nrz(N_MULTI // 5 + 8, sps, 100 + c, offset=((c * 5) % 13 - 6) * 0.0007, smooth=1 + c % 4, noise=0.05 + 0.03 * (c % 5))[:N_MULTI]
        if c == 2:
            x = sm.with_specials(x, 7, 150)
        if c == 3:
            x = sm.with_gap(x, 600, 3000)[:N_MULTI]
    assert len(x) == N_MULTI
    m = sm.SymbolSync(*sm.ADAPTIVE_9600)
    syms, clk, _ = m.run(x)
    if c == 3:
        assert m.max_fold_iters > 500
    x.setflags(write=False)
    return x, syms, clk, m.state()


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("nstreams", [1, 2, 63, 64, 65, 130])
def test_every_row_equals_the_model_run_alone(nstreams, lanes):
    x = np.stack([row(c)[0] for c in range(nstreams)])
    with rr.build_options(sync_lanes=lanes):
        h = rr.SymbolSync(*sm.ADAPTIVE_9600, nstreams=nstreams)
    assert h.streams_per_wave == lanes
    counts, syms, clk = dev_push(h, x, in_stride=N_MULTI + 3, out_stride=N_MULTI + 5)
    for c in range(nstreams):
        _, ws, wc, wstate = row(c)
        assert counts[c] == len(ws), c
        assert np.array_equal(u32(syms[c]), u32(ws)) and np.array_equal(u32(clk[c]), u32(wc)), c
    for c in sorted({0, 1, 2, 3, nstreams - 1} & set(range(nstreams))):
        assert sm.states_equal(h.state(c), row(c)[3]), c
    if nstreams > 1:
        assert counts[1] == len(row(1)[1]) and np.all(u32(syms[1]) == 0)      # the all-zero row still emits, at the free-running clock
    # a second push continues every row where the first left it
    counts2, _, _ = dev_push(h, x[:, :64], in_stride=64, out_stride=64)
    m = sm.SymbolSync(*sm.ADAPTIVE_9600)
    m.run(row(0)[0])
    assert counts2[0] == len(m.run(row(0)[0][:64])[0]) and sm.states_equal(h.state(0), m.state())


def test_the_default_mapping_is_one_of_the_two():
    assert rr.SymbolSync(*sm.AX25_9600, nstreams=32).streams_per_wave in (1, 64)
    with pytest.raises(ValueError, match="sync_lanes"):
        with rr.build_options(sync_lanes=32):
            rr.SymbolSync(*sm.AX25_9600)


# ---- 6. no clock output -----------------------------------------------------------------------------------------------------------------
def test_without_a_clock_output_the_symbols_are_the_same():
    x = np.stack([row(c)[0] for c in range(5)])
    h = rr.SymbolSync(*sm.ADAPTIVE_9600, nstreams=5)
    counts, syms, clk = dev_push(h, x, clock=False)
    assert clk is None
    for c in range(5):
        assert counts[c] == len(row(c)[1]) and np.array_equal(u32(syms[c]), u32(row(c)[1])), c


# ---- 7. the host path --------------------------------------------------------------------------------------------------------------------
def test_host_path_on_pageable_arrays_equals_the_device_path():
    x = np.stack([row(c)[0] for c in range(4)])
    h = rr.SymbolSync(*sm.ADAPTIVE_9600, nstreams=4)
    syms, clk = h.push(x[:, :3000])
    m = [sm.SymbolSync(*sm.ADAPTIVE_9600) for _ in range(4)]
    for c in range(4):
        ws, wc, _ = m[c].run(x[c, :3000])
        assert np.array_equal(u32(syms[c]), u32(ws)) and np.array_equal(u32(clk[c]), u32(wc)), c
    assert h.produced().tolist() == [len(s) for s in syms]
    syms, clk = h.push(np.zeros((4, 0), np.float32))           # n == 0: nothing produced, nothing changed
    assert [len(s) for s in syms] == [0] * 4 and h.produced().tolist() == [0] * 4
    syms, clk = h.push(x[:, 3000:], clock=False)
    assert clk is None
    for c in range(4):
        assert np.array_equal(u32(syms[c]), u32(m[c].run(x[c, 3000:])[0])), c
        assert sm.states_equal(h.state(c), row(c)[3]), c
    # strides wider than n, and sentinels beyond the counts, through the raw entry point
    n, ist, ost = 1000, 1003, 1005
    hin = np.full((4, ist), 1.0, np.float32)
    hin[:, :n] = x[:, :n]
    out_s, out_c = np.full((4, ost), SENTINEL, np.float32), np.full((4, ost), SENTINEL, np.float32)
    produced = (C.c_size_t * 4)()
    h2 = rr.SymbolSync(*sm.ADAPTIVE_9600, nstreams=4)
    assert rr.lib().rr_symbol_sync_push(h2._h, hin.ctypes.data_as(C.c_void_p), ist, n, out_s.ctypes.data_as(C.c_void_p),
                                        out_c.ctypes.data_as(C.c_void_p), ost, produced) == 0
    for c in range(4):
        ws, wc, _ = sm.SymbolSync(*sm.ADAPTIVE_9600).run(x[c, :n])
        k = produced[c]
        assert k == len(ws) and np.array_equal(u32(out_s[c, :k]), u32(ws)) and np.array_equal(u32(out_c[c, :k]), u32(wc))
        assert np.all(u32(out_s[c, k:]) == u32(SENTINEL)) and np.all(u32(out_c[c, k:]) == u32(SENTINEL))


def test_push_errors():
    h = rr.SymbolSync(4.0, 1.0, [1.0], nstreams=2)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    for args, sentence in (((d.data_ptr(), 9, 10, d.data_ptr(), None, 10), "in_stride below n"),
                           ((d.data_ptr(), 10, 10, d.data_ptr(), None, 9), "out_stride below n"),
                           ((d.data_ptr(), 1 << 31, 1 << 31, d.data_ptr(), None, 1 << 31), "2\\^31 samples or more"),
                           ((0, 10, 10, d.data_ptr(), None, 10), "null buffer")):
        with pytest.raises(ValueError, match=sentence):
            h.push_dev(*args)
    h.push_dev(0, 0, 0, 0, None, 0)                           # n == 0 is a valid push
    assert h.produced().tolist() == [0, 0]


# ---- 8. the chain on the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [sm.AX25_1200, sm.ADAPTIVE_9600], ids=["1200", "adaptive-9600"])
def test_receive_chain_on_the_device(prm):
    """HdlcFramer levels held over sps -> SymbolSync -> BitDecoder(nrzi, G3RUH) -> HdlcDeframer(10, 1500), everything behind the
    upload on the device: the frames are those of the same chain with the model in SymbolSync's place, and the packets"""
    rng = np.random.default_rng(8)
    packets = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(8)]
    levels = rr.HdlcFramer(rr.FRAME_FCS | rr.FRAME_G3RUH | rr.FRAME_NRZI | rr.FRAME_SYMBOLS, -1.0, 1.0).push(packets)
    x = sm.hold(levels, prm[0])
    # the precondition on the inputs: with these parameters the MODEL recovers every symbol
    msyms, _, _ = sm.SymbolSync(*prm).run(x)
    assert len(msyms) == len(levels) and np.array_equal(msyms > 0, levels > 0)

    def rest_of_chain(d_syms, count):
        bits = torch.zeros(max(count, 1), dtype=torch.uint8, device="cuda")
        dec = rr.BitDecoder(nrzi=True, descrambler=(0x21, 0, 16))
        assert dec.work_dev(d_syms.data_ptr(), count, bits.data_ptr(), count)[2] == count
        de = rr.HdlcDeframer(10, 1500)
        de.push_dev(bits.data_ptr(), count)
        return [f[1] for f in de.result()]

    d_x = torch.from_numpy(x).cuda()
    d_syms = torch.zeros(len(x), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h = rr.SymbolSync(*prm)
    h.push_dev(d_x.data_ptr(), len(x), len(x), d_syms.data_ptr(), None, len(x))
    count = int(h.produced()[0])
    assert count == len(msyms) and np.array_equal(u32(d_syms[:count].cpu().numpy()), u32(msyms))
    got = rest_of_chain(d_syms, count)
    want = rest_of_chain(torch.from_numpy(msyms.copy()).cuda(), len(msyms))
    assert got == want and got == packets
