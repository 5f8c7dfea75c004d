"""GPU: rr.AddConst (add_const.rs:51-68), Float and Complex: bit-equal to numpy's f32 add over windows of 1, 63, 64, 65 and 100,000
samples, the sync blocks' rr_block_work protocol (the oracle's MultiplyConst runs the same macro), the tag rule, device windows."""
import ctypes as C

import numpy as np
import pytest
import torch

import rustradio_amd as rr
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 100_000]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _floats(rng, n):
    """uniform values with the awkward ones in front: -0.0, +0.0, a denormal, +-Inf, NaN, the negated constant"""
    x = rng.uniform(-4, 4, n).astype(np.float32)
    sp = np.array([-0.0, 0.0, 1e-40, np.inf, -np.inf, np.nan, -0.37], np.float32)
    x[:min(n, len(sp))] = sp[:min(n, len(sp))]
    return x


@pytest.mark.parametrize("n", SIZES)
def test_float_is_numpys_f32_add(n):
    x = _floats(np.random.default_rng(n), n)
    st, c, p, need, y = rr.AddConst(0.37).work(x, n)
    assert (c, p) == (n, n) and y.dtype == np.float32
    assert np.array_equal(_bits(y), _bits(x + np.float32(0.37)))


@pytest.mark.parametrize("n", SIZES)
def test_complex_is_numpys_f32_add_per_component(n):
    rng = np.random.default_rng(1000 + n)
    z = np.empty(n, np.complex64)
    z.real, z.imag = _floats(rng, n), _floats(rng, n)[::-1]
    v = np.complex64(0.6 - 1.25j)
    st, c, p, need, y = rr.AddConst(v, np.complex64).work(z, n)
    assert (c, p) == (n, n) and y.dtype == np.complex64
    want = np.empty(n, np.complex64)
    want.real, want.imag = z.real + np.float32(0.6), z.imag + np.float32(-1.25)
    assert np.array_equal(_bits(y), _bits(want))


@pytest.mark.parametrize("in_len,cap", [(0, 10), (10, 0), (10, 10), (10, 4), (4, 10), (1, 1)])
def test_work_protocol_is_the_sync_macros(in_len, cap):
    """status, consumed, produced, need: what the oracle's sync block answers for the same windows"""
    x = np.arange(in_len, dtype=np.float32)
    st, c, p, need, y = rr.AddConst(2.0).work(x, cap)
    st2, c2, p2, need2, _ = orc.MultiplyConst(2.0).work(x, cap)
    assert (st, c, p, need) == (st2, c2, p2, need2)
    assert c == p == min(in_len, cap) and np.array_equal(y, x[:p] + np.float32(2.0))


def test_tags_are_forwarded_and_the_name():
    for blk in (rr.AddConst(1.0), rr.AddConst(1j, np.complex64)):
        p = C.c_size_t(0)
        assert rr.lib().rr_block_tag_rule(blk._h, C.byref(p)) == 1 and p.value == 1       # RR_TAGS_FORWARD, position for position
        assert blk.name == "AddConst"


def test_device_windows():
    n = 100_003
    x = np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    dy = torch.full((n + 8,), -7.5, dtype=torch.float32, device="cuda")
    b = rr.AddConst(-1700.0 * 2.0 * np.pi / 12000.0)
    st, c, p, need = b.work_dev(dx.data_ptr(), n, dy.data_ptr(), n)
    b.sync()
    y = dy.cpu().numpy()
    assert (c, p) == (n, n) and np.all(y[n:] == -7.5)
    assert np.array_equal(_bits(y[:n]), _bits(x + np.float32(-1700.0 * 2.0 * np.pi / 12000.0)))
