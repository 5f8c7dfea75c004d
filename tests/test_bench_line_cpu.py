"""CPU: the size / strictness guard of bench.py's stdout line (round 5's 22 KB line left the driver's
record with parsed = null).  compact_line() drops the optional tables, largest first, until the line fits 4,000 bytes, and
refuses NaN / Infinity; _clean() turns non-finite floats (and numpy scalars) into null for both the line and the detail file."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench as b
    finally:
        sys.argv = argv
    return b


def _line(n_others):
    return {"metric": "m", "value": 1.0, "unit": "Msamples/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 0.3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "w" * 110}, "roofline": {"bound": "hbm", "frac": 0.6}, "cpu_baseline": {"value": 90.0},
            "metric_chain": {"value": 1.0}, "north_star_target": {"ratio": 1.0}, "parity": {"tol": 1e-5},
            "verified": {"ok": True}, "verified_worst": {"max_err": 1e-7},
            "others_brief": {f"workload_{i}": [1.0, 2.0, 0.5, 0.25] for i in range(n_others)}, "detail": "gpurun_out/bench_detail.json"}


def test_line_fits_and_is_strict(bench):
    s = bench.compact_line(_line(17))
    assert len(s.encode()) <= bench.LINE_LIMIT < 4096 and "others_brief" in json.loads(s)
    # far too many workloads: the optional table goes, the contract keys stay
    s = bench.compact_line(_line(400))
    d = json.loads(s)
    assert len(s.encode()) <= bench.LINE_LIMIT and "others_brief" not in d
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k


def test_non_finite_values_never_reach_the_line(bench):
    bad = _line(3)
    bad["roofline"]["frac"] = float("nan")
    with pytest.raises(ValueError):
        bench.compact_line(bad)                               # json.dumps(allow_nan=False)
    ok = bench._clean({"a": float("nan"), "b": [float("inf"), 1.5, np.float32(2.0), np.int64(3)], "c": {"d": -float("inf")}})
    assert ok == {"a": None, "b": [None, 1.5, 2.0, 3], "c": {"d": None}}
    json.dumps(ok, allow_nan=False)
    assert json.loads(bench.compact_line(bench._clean(bad)))["roofline"]["frac"] is None


class _Block:
    def __init__(self, out_dtype):
        self.out_dtype = out_dtype


class _Workload:
    """the fields of bench_workloads.Workload that dump_outputs reads, on host tensors"""
    def __init__(self, out_dtype, out, cap, produced, windows=1):
        self.blocks, self.bufs, self.caps, self.last_p, self.n_windows = [_Block(out_dtype)], [None, out], [cap], produced, windows


def test_dump_positions_are_fixed_and_spread(bench):
    assert np.array_equal(bench.dump_positions(10, 20), np.arange(10))
    a, b = bench.dump_positions(1_000_003, 1000), bench.dump_positions(1_000_003, 1000)
    assert np.array_equal(a, b) and len(a) == 1000 and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 1_000_003
    assert np.all(a // 1000 == np.arange(1000))                # one position per stride of p // k


def test_dump_outputs_whole_and_sampled(bench, tmp_path):
    import torch
    # real output, 3 windows of capacity 50, 40 produced per window: fits, so every produced element is written
    out = torch.arange(150, dtype=torch.float32)
    bench.dump_outputs(_Workload(np.float32, out, 50, 40, 3), str(tmp_path / "f"), limit=1 << 20)
    y = np.load(tmp_path / "f" / "output.npy")
    assert y.dtype == np.float32 and y.shape == (3, 40)
    assert np.array_equal(y, np.stack([np.arange(c * 50, c * 50 + 40) for c in range(3)]).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "f" / "output_index.npy"), np.arange(40.0))
    assert np.array_equal(np.load(tmp_path / "f" / "output_produced.npy"), np.full(3, 40.0))
    # complex output over the limit: a seeded sample of positions, (re, im) pairs, and the files stay within the limit
    n = 100_000
    out = torch.arange(2 * n, dtype=torch.float32)
    limit = 64 * 1024
    paths = bench.dump_outputs(_Workload(np.complex64, out, n, n - 7), str(tmp_path / "c"), prefix="rank0_", limit=limit)
    assert sorted(os.path.basename(p) for p in paths) == ["rank0_output.npy", "rank0_output_index.npy", "rank0_output_produced.npy"]
    assert sum(os.path.getsize(p) for p in paths) <= limit
    y, pos = np.load(tmp_path / "c" / "rank0_output.npy"), np.load(tmp_path / "c" / "rank0_output_index.npy")
    assert y.dtype == np.float32 and pos.dtype == np.float64 and y.shape == (1, len(pos), 2) and 1000 < len(pos) < n
    assert np.array_equal(pos, bench.dump_positions(n - 7, len(pos)).astype(np.float64))
    assert np.array_equal(y[0, :, 0], 2 * pos) and np.array_equal(y[0, :, 1], 2 * pos + 1)
