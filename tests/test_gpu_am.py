"""GPU: rr.AmDemod (kernels_am.hip) against the float64 definition and the host twin of tests/am_model.py — the bound, the bits
under splits, stream independence, the NaN set, counts and launches — rr.AirspyDecode bit for bit, and three AM stations from one
AirSPY stream down to audio, wholly on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import am_dev as ad
import am_model as am
import rustradio_amd as rr
import rx_chain_helpers as rc
from symsync_dev import SENTINEL, u32

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (289, 1, 1), (289, 3, 7), (33, 5, 2), (9, 1, 1000), (12045, 12, 625), (16384, 1, 1)]
SCALE = 0.5


def _id(s):
    return f"L{s[0]}-{s[1]}to{s[2]}"


def _tile(L, I, D):
    return rr.AmDemod(1, am.taps_for(L), I, D, SCALE).dims()[0]


@pytest.fixture(scope="module")
def refs():
    """per shape: T, the 3 rows of 2T + 3 outputs' worth of samples, and their float64 chains — computed once, left unchanged"""
    memo = {}

    def get(shape):
        if shape not in memo:
            L, I, D = shape
            T = _tile(L, I, D)
            n = am.samples_for_outputs(2 * T + 3, I, D)
            x = np.stack([am.am_signal(n, 20 + c, amp=(1.0, 30.0, 0.02)[c]) for c in range(3)])
            x.setflags(write=False)
            taps = am.taps_for(L)
            memo[shape] = (T, x, taps, [am.chain_f64(x[c], taps, I, D, SCALE) for c in range(3)])
        return memo[shape]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_within_the_bound_of_float64(refs, shape):
    """used <= 1 at output counts T - 1, T, T + 1 and 2T + 3 (with I > D a count comes in steps above one: the first count that
    reaches each), with 1 and 3 streams (the chain is causal: a shorter run's reference is the longer one's prefix)"""
    L, I, D = shape
    T, x, taps, ref = refs(shape)
    h = rr.AmDemod(1, taps, I, D, SCALE)
    assert h.dims() == (T, L - 1)
    worst = 0.0
    for asked in (T - 1, T, T + 1, 2 * T + 3):
        n = am.samples_for_outputs(asked, I, D)
        k = am.count(n, I, D)
        assert 0 <= k - asked < max(1, -(-I // D))            # exactly the count asked for unless I > D
        for ns in (1, 3):
            got = ad.dev_push(rr.AmDemod(ns, taps, I, D, SCALE), x[:ns, :n])
            assert got.shape == (ns, k)
            for c in range(ns):
                u = am.used(got[c], {key: v[:k] for key, v in ref[c].items()}, L, SCALE)
                worst = max(worst, u)
                assert u <= 1.0, (k, ns, c, u)
    print(f"{_id(shape)}: T {T}, used {worst:.4f}")


@pytest.mark.parametrize("shape", [(289, 3, 7), (9, 1, 1000), (12045, 12, 625)], ids=_id)
def test_device_equals_the_host_twin(refs, shape):
    """bit for bit: am_host.hpp's twin (tests/cpp/emu_am.cpp) takes am_core.hpp with the kernel's indexing, on the CPU"""
    L, I, D = shape
    T, x, taps, _ = refs(shape)
    got = ad.dev_push(rr.AmDemod(3, taps, I, D, SCALE), x)
    want = am.twin(x, taps, I, D, SCALE)
    assert ad.same_bits(got, want)


@pytest.mark.parametrize("shape", [(289, 3, 7), (33, 5, 2), (9, 1, 1000)], ids=_id)
def test_split_invariance(refs, shape):
    """one push == ragged cuts, cuts inside the first L - 1 samples, a cut exactly on a tile's last output, and (D >> I) pushes
    that produce no output — bit for bit"""
    L, I, D = shape
    T, x, taps, _ = refs(shape)
    n = x.shape[1]
    whole = ad.dev_push(rr.AmDemod(3, taps, I, D, SCALE), x)
    at_tile = am.samples_for_outputs(T, I, D)                 # the first T outputs exist after exactly this many samples
    early = max(1, (L - 1) // 2)
    cuts = [rc.ragged_cuts(n), [early, 1, 0, n - early - 1], [at_tile, n - at_tile], [at_tile - 1, 1, 1, n - at_tile - 1]]
    if D > 2 * I:
        cuts.append([1, 1, 1, n - 3])                         # behind the first, a 1-sample push produces nothing
    for lens in cuts:
        h = rr.AmDemod(3, taps, I, D, SCALE)
        got = ad.run_pushes(h, x, lens)
        assert ad.same_bits(got, whole), lens
    if D > 2 * I:
        h = rr.AmDemod(1, taps, I, D, SCALE)
        assert ad.dev_push(h, x[:1, :1]).shape == (1, 1) and ad.dev_push(h, x[:1, 1:2]).shape == (1, 0)


def test_streams_do_not_see_each_other():
    """row c of a 5-stream handle == a 1-stream handle fed row c, amplitudes 10^4 apart"""
    L, I, D = 289, 3, 7
    taps = am.taps_for(L)
    T = _tile(L, I, D)
    n = am.samples_for_outputs(T + 7, I, D)
    x = np.stack([am.am_signal(n, 40 + c, amp=a) for c, a in enumerate((1e-4, 1.0, 1e4, 1e-8, 1e8))])
    got = ad.run_pushes(rr.AmDemod(5, taps, I, D, SCALE), x, [n // 2, n - n // 2])
    for c in range(5):
        alone = ad.run_pushes(rr.AmDemod(1, taps, I, D, SCALE), x[c], [n // 2, n - n // 2])
        assert ad.same_bits(got[c:c + 1], alone), c


@pytest.mark.parametrize("shape", [(289, 3, 7), (33, 5, 2)], ids=_id)
def test_nan_reaches_exactly_its_outputs(refs, shape):
    """one NaN at k in {0, L - 1, the sample under the last output of tile 0, the last sample}: exactly the outputs whose window
    holds it are NaN, every other bit is the clean run's — also when the NaN arrives in one push and its outputs in the next"""
    L, I, D = shape
    T, x, taps, _ = refs(shape)
    x = x[:1]
    n = x.shape[1]
    clean = ad.dev_push(rr.AmDemod(1, taps, I, D, SCALE), x)
    n_out = clean.shape[1]
    under = int(am.picks(T, I, D)[T - 1])
    for k in (0, L - 1, under, n - 1):
        for part in ("re", "im"):
            bad = x.copy()
            bad[0, k] = complex(np.nan, 1.0) if part == "re" else complex(1.0, np.nan)
            want = am.nan_set(k, n_out, L, I, D)
            assert want.any()
            runs = [[n]]
            if 0 < k + 1 < n:
                runs.append([k + 1, n - k - 1])               # the NaN is the last sample of a push
            for lens in runs:
                got = ad.run_pushes(rr.AmDemod(1, taps, I, D, SCALE), bad, lens)
                assert np.array_equal(np.isnan(got[0]), want), (k, lens)
                assert np.array_equal(u32(got[0])[~want], u32(clean[0])[~want]), (k, lens)


def test_counts_follow_the_lengths():
    """produced == ceil((N0 + n) I / D) - ceil(N0 I / D) over 50 random pushes (ad.dev_push asserts each), and the whole equals one push"""
    L, I, D = 33, 3, 7
    taps = am.taps_for(L)
    rng = np.random.default_rng(11)
    lens = [int(v) for v in rng.integers(0, 400, 50)]
    x = np.stack([am.am_signal(sum(lens), 60 + c) for c in range(2)])
    h = rr.AmDemod(2, taps, I, D, SCALE)
    got = ad.run_pushes(h, x, lens)
    assert h.total == sum(lens) and got.shape == (2, am.count(sum(lens), I, D))
    assert ad.same_bits(got, ad.dev_push(rr.AmDemod(2, taps, I, D, SCALE), x))


@pytest.mark.parametrize("ns", [1, 4096])
def test_one_launch_per_push(ns):
    L, I, D = 9, 2, 3
    taps = am.taps_for(L)
    x = np.repeat(am.am_signal(64, 70)[None, :], ns, axis=0)
    h = rr.AmDemod(ns, taps, I, D, SCALE)
    d_in = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    d_out = torch.zeros((ns, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for n in (1, 64, 0, 7):
        before = ad.launches()
        h.push_dev(d_in.data_ptr(), 64, n, d_out.data_ptr(), 64)
        assert ad.launches() - before == (1 if n else 0), n
    h.sync()


def test_refused_pushes_launch_nothing_and_change_nothing():
    L, I, D = 33, 5, 2
    taps = am.taps_for(L)
    x = np.stack([am.am_signal(300, 80 + c) for c in range(2)])
    whole = ad.dev_push(rr.AmDemod(2, taps, I, D, SCALE), x)
    h = rr.AmDemod(2, taps, I, D, SCALE)
    first = ad.dev_push(h, x[:, :100])
    d_in = torch.from_numpy(np.ascontiguousarray(x[:, 100:]).view(np.float32)).cuda()
    d_out = torch.from_numpy(np.full((2, 600), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    k = h.count(200)
    assert k == 500
    refusals = [((d_in.data_ptr(), 199, 200, d_out.data_ptr(), 600), "in_stride below n"),
                ((d_in.data_ptr(), 200, 200, d_out.data_ptr(), k - 1), "out_stride below produced"),
                ((0, 200, 200, d_out.data_ptr(), 600), "null buffer"),
                ((d_in.data_ptr(), 200, 200, 0, 600), "null buffer"),
                ((d_in.data_ptr(), 1 << 30, 1 << 30, d_out.data_ptr(), 1 << 32), "more than 2\\^30 samples")]
    for args, msg in refusals:
        before = ad.launches()
        with pytest.raises(ValueError, match=msg):
            h.push_dev(*args)
        assert ad.launches() == before and h.total == 100
    with pytest.raises(RuntimeError, match="rr_am_demod_push"):
        h.work(x[0], 10)                                      # a batch block: no stream protocol
    h.sync()
    assert np.all(u32(d_out.cpu().numpy()) == u32(SENTINEL))
    rest = ad.dev_push(h, x[:, 100:])
    assert ad.same_bits(np.concatenate([first, rest], axis=1), whole)


def test_host_push_equals_device_push():
    L, I, D = 289, 3, 7
    taps = am.taps_for(L)
    x = np.stack([am.am_signal(1500, 90 + c) for c in range(3)])
    h = rr.AmDemod(3, taps, I, D, SCALE)
    got = np.concatenate([h.push(x[:, :1]), h.push(x[:, 1:1]), h.push(x[:, 1:700]), h.push(x[:, 700:])], axis=1)
    assert ad.same_bits(got, ad.dev_push(rr.AmDemod(3, taps, I, D, SCALE), x))


# ---- AirspyDecode --------------------------------------------------------------------------------------------------------------------
def _words(i16, q16):
    return np.asarray(i16, np.int16).view(np.uint16).astype(np.uint32) | (np.asarray(q16, np.int16).view(np.uint16).astype(np.uint32) << 16)


def _decoded(i16, q16):
    return np.asarray(i16, np.int16).astype(np.float32) / np.float32(1000), np.asarray(q16, np.int16).astype(np.float32) / np.float32(1000)


def test_airspy_decode_every_value():
    """bit-exact against int16 -> float32 / float32(1000): all 65,536 values of I at fixed Q, and the reverse"""
    v = np.arange(-32768, 32768).astype(np.int16)
    for fixed in (-32768, -1, 0, 12345):
        f = np.full_like(v, fixed)
        for i16, q16 in ((v, f), (f, v)):
            st, c, p, need, y = rr.AirspyDecode().work(_words(i16, q16), len(v))
            assert (c, p) == (len(v), len(v))
            re, im = _decoded(i16, q16)
            assert np.array_equal(u32(y.real), u32(re)) and np.array_equal(u32(y.imag), u32(im))


def test_airspy_decode_protocol_and_tags():
    """the sync protocol's counts for in < out, in > out and empty windows; tags forwarded like ComplexToMag2"""
    blk = rr.AirspyDecode()
    w = _words(np.arange(100), -np.arange(100))
    assert blk.work(w, 300)[:4] == (rr.WAIT_SRC, 100, 100, 1)
    assert blk.work(w, 40)[:4] == (rr.WAIT_DST, 40, 40, 1)
    assert blk.work(w, 100)[:4] == (rr.WAIT_SRC, 100, 100, 1)
    assert blk.work(w[:0], 10)[:4] == (rr.WAIT_SRC, 0, 0, 1)
    assert blk.work(w, 0)[:4] == (rr.WAIT_DST, 0, 0, 1)
    p, q = C.c_size_t(0), C.c_size_t(0)
    ref = rr.ComplexToMag2()
    assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == rr.lib().rr_block_tag_rule(ref._h, C.byref(q)) == 1 and p.value == q.value == 1
    assert blk.name == "AirspyDecode"
    assert rr.lib().rr_block_in_elem_size(blk._h) == 4 and rr.lib().rr_block_out_elem_size(blk._h) == 8
    assert blk.eof(True) and not blk.eof(False)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_three_am_stations_from_one_airspy_stream():
    """AirspyDecode -> Channelizer(3 channels, 257 taps, 1:12) -> AmDemod(129 taps, 1:5), device buffers only: each channel's
    audio, mean removed, correlates above 0.99 with its own station's tone and below 0.2 with the other two"""
    words, _ = am.e2e_iq()
    n = len(words)
    dec, chan = rr.AirspyDecode(), rr.Channelizer(am.e2e_rf_taps(), 1, am.E2E_DECI)
    dem = rr.AmDemod(3, am.e2e_audio_taps(), *am.E2E_AUDIO, 1.0)
    cap = n // am.E2E_DECI + 64
    d_w = torch.from_numpy(words.view(np.int32).copy()).cuda()
    d_x = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_ch = torch.zeros(3 * cap * 2, dtype=torch.float32, device="cuda")
    acap = cap // am.E2E_AUDIO[1] + 8
    d_audio = torch.from_numpy(np.full((3, acap), SENTINEL, np.float32)).cuda()
    torch.cuda.synchronize()
    st, c, p, need = dec.work_dev(d_w.data_ptr(), n, d_x.data_ptr(), n)
    assert (c, p) == (n, n)
    parts, pos = [], 0
    for _ in range(100):
        st, c, p, need = chan.work_dev(d_x.data_ptr() + 8 * pos, n - pos, d_ch.data_ptr(), cap)
        pos += c
        if p:
            k = dem.push_dev(d_ch.data_ptr(), cap, p, d_audio.data_ptr(), acap)
            dem.sync()
            parts.append(d_audio.cpu().numpy()[:, :k].copy())
        if not c and not p:
            break
    audio = np.concatenate(parts, axis=1)
    model = am.e2e_model()
    assert model.shape[1] * 0.7 < audio.shape[1] <= model.shape[1] and np.all(np.isfinite(audio))
    s = am.e2e_scores(audio)
    print(np.round(s, 4))
    for ch in range(3):
        for t in range(3):
            assert (s[ch, t] > 0.99) if ch == t else (s[ch, t] < 0.2), (ch, t, s[ch, t])
