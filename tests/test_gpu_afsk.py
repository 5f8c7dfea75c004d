"""GPU: rr.AfskDemod (kernels_afsk.hip) against the float64 form of its definition (tests/afsk_model.py) within the propagated
bound, stream independence and split invariance bit for bit, the launch count, the refusals, the host-pointer push, and the
1200-baud receiver end to end on device pointers: AfskDemod -> SymbolSync -> HdlcReceiver."""
import numpy as np
import pytest
import torch

import afsk_dev as ad
import afsk_model as am
import rustradio_amd as rr

pytestmark = pytest.mark.gpu
TILE = 2048


def stream0():
    return torch.cuda.current_stream().cuda_stream


def test_dims():
    h = rr.AfskDemod(3, 65, am.lp_taps(289))
    assert h.dims() == (TILE, 289 + 65)
    with pytest.raises(RuntimeError, match="AfskDemod runs nstreams streams"):
        h.work(np.zeros(8, np.float32), 8)


def test_parity_on_the_sixteen_stream_signal():
    """one push of the padded rows: every stream within the bound of float64, `used` printed"""
    x, _ = am.samples()
    taps = am.taps12k()
    h = rr.AfskDemod(am.NSTREAMS, am.HIL, taps, am.GAIN, am.OFFSET)
    got = ad.dev_push(h, x)
    assert got.shape == (am.NSTREAMS, x.shape[1] - 1)
    worst = max(am.used(got[c], am.reference(c), am.GAIN, taps) for c in range(am.NSTREAMS))
    print(f"16 x {x.shape[1]}: used {worst:.4f}")
    assert worst <= 1.0


SHAPES = [(3, 1, 1), (65, 2, 1), (65, 1205, 1), (65, TILE + 1, 1), (65, 289, 2), (65, 289, 65)]


@pytest.mark.parametrize("H,L,ns", SHAPES, ids=[f"H{h}-L{l}-N{s}" for h, l, s in SHAPES])
def test_parity_on_two_tone_rows(H, L, ns):
    """2 tile + 3 samples, the smallest n that crosses a tile twice: within the bound of float64 on every stream; and the host
    pointers' push gives the bits of the device pointers'"""
    n = 2 * TILE + 3
    x = np.stack([am.two_tone(n, c) for c in range(ns)])
    hil, taps, gain, off = am.hilbert(H), am.lp_taps(L), 1.0, -0.25
    got = ad.dev_push(rr.AfskDemod(ns, H, taps, gain, off), x)
    assert got.shape == (ns, n - 1)
    worst = max(am.used(got[c], am.chain_f64(x[c], hil, gain, taps, off), gain, taps) for c in range(ns))
    print(f"H {H} L {L} x {ns}: used {worst:.4f}")
    assert worst <= 1.0
    assert ad.same_bits(rr.AfskDemod(ns, H, taps, gain, off).push(x), got)


def test_stream_independence():
    """row c of 65 streams == a 1-stream handle fed row c, bit for bit (rows of different amplitude and tones)"""
    n, ns = 2 * TILE + 3, 65
    x = np.stack([(0.2 + 0.01 * c) * am.two_tone(n, c) for c in range(ns)])
    taps = am.lp_taps(289)
    got = ad.dev_push(rr.AfskDemod(ns, 65, taps, 1.0, 0.5), x)
    for c in (0, 1, 31, 63, 64):
        assert ad.same_bits(ad.dev_push(rr.AfskDemod(1, 65, taps, 1.0, 0.5), x[c]), got[c:c + 1]), c


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_over_splits_and_taps(seed):
    """seeded: H, L, stream count, gain, offset and the cuts (0- and 1-sample pushes among them) drawn at random; any split gives
    the bits of one push, within the bound of float64"""
    rng = np.random.default_rng(9100 + seed)
    H = int(rng.choice([3, 5, 33, 65, 129]))
    L = int(rng.choice([1, 2, 7, 8, 9, 64, 289, 700, TILE - 1]))
    ns = int(rng.integers(1, 5))
    n = int(rng.integers(TILE, 3 * TILE))
    gain, off = float(rng.uniform(0.5, 2.0)), float(rng.uniform(-1, 1))
    x = np.stack([am.two_tone(n, 100 * seed + c) for c in range(ns)])
    hil, taps = am.hilbert(H), am.lp_taps(L)
    whole = ad.dev_push(rr.AfskDemod(ns, H, taps, gain, off), x)
    at = np.sort(rng.integers(0, n + 1, int(rng.integers(1, 7))))
    lens = [int(v) for v in np.diff(np.concatenate([[0], at, [n]]))]
    lens[-1:] = [1, 0, lens[-1] - 1] if lens[-1] > 1 else lens[-1:]
    assert ad.same_bits(ad.run_pushes(rr.AfskDemod(ns, H, taps, gain, off), x, lens), whole), (H, L, ns, lens)
    worst = max(am.used(whole[c], am.chain_f64(x[c], hil, gain, taps, off), gain, taps) for c in range(ns))
    print(f"seed {seed}: H {H} L {L} x {ns} n {n} cuts {lens}: used {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("ns,n", [(1, 3 * TILE), (4096, 70)])
def test_one_launch_per_push(ns, n):
    """one launch whatever nstreams and n are — the carry is written by the last tile — and none for an empty push"""
    h = rr.AfskDemod(ns, 65, am.lp_taps(33))
    d_in = torch.zeros((ns, n), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((ns, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, want in ((n, 1), (0, 0), (1, 1), (n, 1)):
        l0 = ad.launches()
        h.push_dev(d_in.data_ptr(), n, k, d_out.data_ptr(), n, stream0())
        assert ad.launches() - l0 == want, (ns, k)
    h.sync()


def test_create_refusals():
    """each with its sentence (tests/test_afsk_cpu.py shows they are said before a device is touched)"""
    ok = dict(nstreams=2, hilbert_ntaps=65, taps=[0.25, 0.5, 0.25])
    for kw, msg in [(dict(nstreams=0), "nstreams out of range"), (dict(nstreams=4097), "nstreams out of range"),
                    (dict(hilbert_ntaps=66), "hilbert filter len must be odd and greater than 1"),
                    (dict(hilbert_ntaps=1), "hilbert filter len must be odd and greater than 1"),
                    (dict(taps=[]), "AfskDemod needs 1 to 4096 finite taps"),
                    (dict(taps=np.ones(4097)), "AfskDemod needs 1 to 4096 finite taps"),
                    (dict(taps=[np.nan]), "AfskDemod needs 1 to 4096 finite taps"),
                    (dict(gain=np.inf), "gain and offset must be finite"), (dict(offset=np.nan), "gain and offset must be finite")]:
        l0 = ad.launches()
        with pytest.raises(ValueError, match=msg):
            rr.AfskDemod(**dict(ok, **kw))
        assert ad.launches() == l0
    assert rr.AfskDemod(4096, 65, np.ones(4096, np.float32)).dims() == (TILE, 4096 + 65)      # the caps themselves are fine


def test_push_refusals_launch_nothing_and_change_nothing():
    ns, n = 3, 500
    x = np.stack([am.two_tone(2 * n, c) for c in range(ns)])
    taps = am.lp_taps(9)
    h = rr.AfskDemod(ns, 5, taps)
    first = ad.dev_push(h, x[:, :n])
    d = torch.zeros((ns, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    l0 = ad.launches()
    for args, msg in [((d.data_ptr(), n - 1, n, d.data_ptr(), n), "in_stride below n"),
                      ((d.data_ptr(), n, n, d.data_ptr(), n - 1), "out_stride below n"),
                      ((0, n, n, d.data_ptr(), n), "null buffer"), ((d.data_ptr(), n, n, 0, n), "null buffer"),
                      ((d.data_ptr(), 1 << 29, 1 << 29, d.data_ptr(), 1 << 29), "more than 2\\^30 samples")]:
        with pytest.raises(ValueError, match=msg):
            h.push_dev(*args)
    assert ad.launches() == l0
    assert h.push_dev(0, 0, 0, 0, 0) == 0 and ad.launches() == l0            # (an empty push needs no buffers)
    second = ad.dev_push(h, x[:, n:])
    whole = ad.dev_push(rr.AfskDemod(ns, 5, taps), x)
    assert ad.same_bits(np.concatenate([first, second], axis=1), whole)


def test_afsk_to_frames_end_to_end(tmp_path):
    """AfskDemod(16) -> SymbolSync(10.0, 0.5, [0.1, 0.9], 16) -> HdlcReceiver(16, nrzi, 1, 60) on device pointers in three pushes on
    one HIP stream: `produced` is SymbolSync's n, counts_dev() goes to the receiver, nothing is read by the host in between.
    Frames == payloads, stats (3, 0, 0) for every stream; the symbol counts of every push are the models' over the host twin's
    soft samples (tests/cpp/emu_afsk.cpp)."""
    x, _ = am.samples()
    N, n = x.shape
    taps, hil = am.taps12k(), am.hilbert(am.HIL)
    cuts = am.cuts(n)
    exe = str(tmp_path / "emu_afsk")
    am.build_emu(exe, ["-O2"])
    twin = np.concatenate(am.run_emu(exe, str(tmp_path), [(x, hil, am.GAIN, taps, am.OFFSET, cuts)])[0], axis=1)
    model = am.chain_model(list(twin), am.soft_cuts(cuts))
    af = rr.AfskDemod(N, am.HIL, taps, am.GAIN, am.OFFSET)
    ss = rr.SymbolSync(*am.SYNC_PRM, nstreams=N)
    rx = rr.HdlcReceiver(N, 1, am.MAX_SIZE, nrzi=True)
    dx = torch.from_numpy(x.copy()).cuda()
    s, at, frames = stream0(), 0, [[] for _ in range(N)]
    for k, want in zip(cuts, model):
        win = dx[:, at:at + k].contiguous()
        soft = torch.zeros((N, k), dtype=torch.float32, device="cuda")
        syms = torch.zeros((N, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        p = af.push_dev(win.data_ptr(), k, k, soft.data_ptr(), k, s)
        assert p == (k if at else k - 1)
        ss.push_dev(soft.data_ptr(), k, p, syms.data_ptr(), None, k, s)
        rx.push_dev(syms.data_ptr(), k, p, ss.counts_dev(), s)
        got = rx.result()                                                       # (waits for all three)
        assert [int(v) for v in ss.produced()] == want["counts"]
        assert got == want["frames"]
        for c in range(N):
            frames[c] += [f[1] for f in got[c]]
        at += k
    assert at == n
    assert all(frames[c] == am.payloads(c) for c in range(N))
    assert [tuple(int(v) for v in r) for r in rx.stats()] == [(3, 0, 0)] * N
