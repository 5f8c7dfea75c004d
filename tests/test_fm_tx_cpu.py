"""CPU-only: the Vco model the GPU tests of rr_vco_create / rr_fm_tx_create rely on (tests/tx_model.py) against the
long-double truth, its carried phase, its non-finite rule — and the public surface of the two blocks."""
import ctypes
import math

import numpy as np
import pytest

import rustradio_amd as rr
from tx_model import bound, comp_err, vco_model, vco_truth

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
