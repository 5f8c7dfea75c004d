"""CPU-only: the Vco model the GPU tests of rr_vco_create / rr_fm_tx_create rely on (tests/tx_model.py) against the
long-double truth, its carried phase, its non-finite rule, the exact truth on a dyadic grid and the bound for large steps
that the long GPU cases are judged with — and the public surface of the two blocks."""
import ctypes
import math

import numpy as np
import pytest

import rustradio_amd as rr
from tx_model import (GRID_G, MX, bound, bound_steps, comp_err, fm_tx_truth, fm_tx_truth_grid, grid_noise, grid_signal,
                      truth_grid_error, vco_model, vco_step_model, vco_truth, vco_truth_grid)

K75 = 2.0 * math.pi * 75000 / 480000
K5 = 2.0 * math.pi * 5000 / 480000
N = 200_000


def _signals():
    rng = np.random.default_rng(20)
    t = np.arange(N, dtype=np.float64)
    return {
        "noise": (rng.uniform(-1, 1, N).astype(np.float32), K75),
        "dc+1": (np.ones(N, np.float32), K75),
        "dc-1": (-np.ones(N, np.float32), K5),
        "tone": (np.sin(2 * np.pi * 1000.0 / 480000.0 * t).astype(np.float32), K5),
    }


@pytest.mark.parametrize("name", ["noise", "dc+1", "dc-1", "tone"])
def test_model_is_within_the_bound_of_the_truth(name):
    a, k = _signals()[name]
    y, _ = vco_model(a, k)
    e = comp_err(y, vco_truth(a, k))
    print(f"{name}: model vs long-double truth {e:.4e}, bound {bound(N):.4e}")
    assert e <= bound(N)


def test_model_carries_the_reference_phase_bit_for_bit():
    rng = np.random.default_rng(21)
    a = rng.uniform(-1, 1, 30_000).astype(np.float32)
    whole, ph_whole = vco_model(a, K75)
    cuts = np.sort(rng.choice(np.arange(1, len(a)), 17, replace=False))
    parts, ph = [], 0.0
    for seg in np.split(a, cuts):
        y, ph = vco_model(seg, K75, ph)
        parts.append(y)
    got = np.concatenate(parts)
    assert got.view(np.uint32).tolist() == whole.view(np.uint32).tolist()
    assert ph == ph_whole


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("p", [0, 5, 999])
def test_model_non_finite_poisons_everything_after(bad, p):
    rng = np.random.default_rng(22)
    a = rng.uniform(-1, 1, 1000).astype(np.float32)
    b = rng.uniform(-1, 1, 300).astype(np.float32)
    clean, _ = vco_model(a, K75)
    a2 = a.copy(); a2[p] = bad
    y1, ph = vco_model(a2, K75)
    y2, _ = vco_model(b, K75, ph)                 # a second call with finite input
    assert y1[:p].view(np.uint32).tolist() == clean[:p].view(np.uint32).tolist()
    for y in (y1[p:], y2):
        assert np.all(np.isnan(y.real)) and np.all(np.isnan(y.imag))


# ---- the exact truth on a dyadic grid, and the bound for large steps ---------------------------------------------------------
def _apart(t, u):
    """largest per-component distance of two truths"""
    return float(max(np.max(np.abs(t.real - u.real)), np.max(np.abs(t.imag - u.imag))))


def test_grid_truth_agrees_with_the_long_double_truth():
    q, a = grid_noise(N, 23)
    assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64) * 4096.0, q.astype(np.float64))   # the grid is exact
    d = _apart(vco_truth_grid(q, GRID_G, K75), vco_truth(a, K75))
    print(f"grid truth vs long-double cumsum, noise: {d:.4e} (own error at most {truth_grid_error(N, K75):.4e})")
    assert d <= 1e-12 and truth_grid_error(N, K75) <= 1e-12
    assert _apart(fm_tx_truth_grid(q[:5000], GRID_G, 7, 5, K75, 7000), fm_tx_truth(a[:5000], 7, 5, K75, 7000)) <= 1e-12


def test_model_is_within_the_bound_of_the_grid_truth_on_dc():
    n = 400_000                                   # 61 times round the circle at K75: where vco_truth's own cumsum starts to drift
    q = np.full(n, 4096, np.int64)
    y, _ = vco_model(grid_signal(q), K75)
    e = comp_err(y, vco_truth_grid(q, GRID_G, K75))
    print(f"dc+1 x {n}: model vs grid truth {e:.4e}, bound {bound(n):.4e}")
    assert e <= bound(n)
    assert truth_grid_error(n, K75) <= 0.01 * bound(n)


_K_LARGE = [10.0, 4.0 * math.pi, 13.0, 100.0, 1e4, 1e6, -1e6]      # 2 pi < |k| <= 4 pi: wrap only; beyond: whole turns removed


@pytest.mark.parametrize("sig", ["noise", "dc+1", "dc-1"])
@pytest.mark.parametrize("k", _K_LARGE)
def test_step_model_is_within_bound_steps(k, sig):
    n = 3 * 2048 + 17
    q = grid_noise(n, 24)[0] if sig == "noise" else np.full(n, 4096 if sig == "dc+1" else -4096, np.int64)
    y, ph = vco_step_model(grid_signal(q), k)
    assert abs(ph) <= MX
    e = comp_err(y, vco_truth_grid(q, GRID_G, k))
    print(f"{sig} k={k}: kernel-rule model vs grid truth {e:.4e}, bound_steps {bound_steps(n, abs(k)):.4e}")
    assert e <= bound_steps(n, abs(k))
    assert truth_grid_error(n, k) <= 0.01 * bound_steps(n, abs(k))


def test_bound_steps_extends_bound_and_bound_is_unchanged():
    for n in (1, 700, 200_000, 4097 * 2048 + 17):
        assert bound(n) == 2.0 ** -25 + n * 2.0 ** -48
        assert bound_steps(n, 0.0) == bound(n)
        for d in (0.5, MX, 13.0, 1e6):
            assert bound_steps(n, d) >= bound(n)
            assert bound_steps(n, d) == 2.0 ** -25 + n * (2.0 ** -48 + d * 2.0 ** -52)
    assert bound(4097 * 2048 + 17) == pytest.approx(5.96e-8, rel=2e-3)


def test_public_surface():
    from rustradio_amd._lib import SYMBOLS
    assert "rr_vco_create" in SYMBOLS and "rr_fm_tx_create" in SYMBOLS
    assert callable(rr.Vco) and callable(rr.FmTx)
    L = rr.lib()
    assert L.rr_vco_create.argtypes == [ctypes.c_ulonglong]                       # k as f64::to_bits
    assert L.rr_fm_tx_create.argtypes == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_ulonglong]
    assert rr.lib().rr_abi_version() == 3
    import torch
    if not torch.cuda.is_available():            # no CPU fallback: constructing either needs a device
        with pytest.raises(ValueError, match="no usable HIP device"):
            rr.Vco(K75)
        with pytest.raises(ValueError, match="no usable HIP device"):
            rr.FmTx(10, 1, K5)
