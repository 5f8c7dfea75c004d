"""No GPU: the arithmetic of rustradio_amd/csrc/symsync_core.hpp run lane by lane on the CPU against the reference's sequential
machine (tests/symsync_model.py), bit for bit; the host-only logic behind the entry points (rustradio_amd/csrc/symsync_host.hpp)
under the host sanitizers; and what rr.SymbolSync says without a device."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import rustradio_amd as rr
import symsync_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rustradio_amd", "csrc")


# ---- the model itself, on the facts the reference fixes -----------------------------------------------------------------------------
def test_model_passes_the_reference_own_test():
    """symbol_sync.rs:229-242: 10 zeros, sps 4, max_deviation 1, taps [1.0] -> 2 symbols (at input indices 2 and 6)"""
    syms, clk, idx = sm.SymbolSync(4.0, 1.0, [1.0]).run(np.zeros(10, np.float32))
    assert len(syms) == 2 and idx.tolist() == [2, 6] and clk.tolist() == [4.0, 4.0]


def test_model_iir_filter_passes_the_reference_own_tests():
    """iir_filter.rs:160-205 (filter_clamped and fill)"""
    f = sm.IirFilter([1.0, 0.0])
    assert [float(f.filter_clamped(sm.F(10.0), sm.F(0.0), sm.F(1.0))) for _ in range(3)] == [1.0, 1.0, 1.0]
    f = sm.IirFilter([1.0, 0.9, 0.1])
    f.fill(100.0)
    big = sm.F(1e9)
    assert [float(f.filter_clamped(sm.F(v), -big, big)) for v in (100.0, 100.0, 200.0)] == [200.0, 290.0, 481.0]


def test_model_is_the_same_for_any_split_into_runs():
    x = sm.nrz(400, sm.AX25_9600[0], 3, offset=0.003, smooth=3, noise=0.1)
    whole = sm.SymbolSync(*sm.AX25_9600)
    a = whole.run(x)
    rng = np.random.default_rng(5)
    parts = sm.SymbolSync(*sm.AX25_9600)
    s, c, pos = [], [], 0
    while pos < len(x):
        k = int(rng.integers(0, 200))
        r = parts.run(x[pos:pos + k])
        s.append(r[0]); c.append(r[1])
        pos += k
    assert sm.bits_equal(np.concatenate(s), a[0]) and sm.bits_equal(np.concatenate(c), a[1])
    assert sm.states_equal(parts.state(), whole.state())
    assert abs(len(a[0]) - 400) <= 2 and whole.clock_updates > 50


# ---- symsync_core.hpp under g++ -ffp-contract=off ----------------------------------------------------------------------------------
def _cases():
    """[(name, (sps, max_deviation, taps), push lengths, samples)]"""
    rng = np.random.default_rng(11)

    def pushes(n, specials=(0, 1, 63, 64, 65)):
        ln = list(specials)
        while sum(ln) < n:
            ln.append(int(rng.integers(0, 400)))
        ln[-1] -= sum(ln) - n
        return ln

    out = [("reference test", (4.0, 1.0, [1.0]), [10], np.zeros(10, np.float32))]
    for name, prm in (("9600", sm.AX25_9600), ("adaptive", sm.ADAPTIVE_9600)):
        x = sm.nrz(600, prm[0], 21, offset=0.003, smooth=3, noise=0.15)
        out.append((name + " one push", prm, [len(x)], x))
        out.append((name + " random pushes", prm, pushes(len(x)), x))
    x = sm.nrz(120, sm.AX25_1200[0], 22, offset=-0.002, smooth=9, noise=0.1)
    out.append(("1200", sm.AX25_1200, pushes(len(x)), x))
    x = sm.nrz(500, 5.0, 23, offset=0.004, noise=0.2)
    out.append(("ntaps 1", (5.0, 0.5, [0.25]), pushes(len(x)), x))
    out.append(("ntaps 8", (5.0, 0.5, [0.05, 0.3, 0.2, 0.15, 0.1, 0.08, 0.07, 0.05]), pushes(len(x)), x))
    out.append(("ntaps 8, max_deviation at sps / 2", (5.0, 2.5, [0.3, 0.3, 0.2, 0.1, 0.05, 0.03, 0.01, 0.01]), pushes(len(x)), x))
    x = sm.with_gap(sm.nrz(300, sm.AX25_9600[0], 24, noise=0.05), 700, 3000)
    out.append(("idle gap", sm.AX25_9600, pushes(len(x)), x))
    x = sm.with_specials(sm.nrz(400, sm.AX25_9600[0], 25, offset=0.002, noise=0.1), 26, 120)
    out.append(("NaN, Inf and signed zeros", sm.ADAPTIVE_9600, pushes(len(x)), x))
    x = sm.nrz(2000, 5.0, 27, noise=0.3)[:sum(range(1, 131))]
    out.append(("a word seam in every position of a window", sm.ADAPTIVE_9600, list(range(1, 131)), x))
    # what tests/test_gpu_symsync_edges.py runs on the device passes here first
    for key, prm in sm.SPS_EDGES.items():
        out.append(("sps " + key, prm, list(sm.SPS_EDGE_PUSHES), sm.sps_edge_signal(key)))
    out.append(("non-finite clock", sm.NONFINITE, [sm.NONFINITE_N], sm.nonfinite_signal()))
    x = sm.with_gap(sm.nrz(400, sm.ADAPTIVE_9600[0], 28, offset=0.002, smooth=3, noise=0.05), 600, (1 << 18) + 1000)
    out.append(("a gap of 2^18 samples", sm.ADAPTIVE_9600, [1, 63, 64, 65, 700, len(x) - 893], x))
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("symsync")
    exe = str(d / "emu_symsync")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "emu_symsync.cpp"),
                    "-o", exe], check=True)
    cases = _cases()
    blob = [struct.pack("<i", len(cases))]
    for _, (sps, dev, taps), lens, x in cases:
        assert sum(lens) == len(x) and min(lens) >= 0
        t = np.zeros(8, np.float32)
        t[:len(taps)] = taps
        blob += [struct.pack("<ffi", sps, dev, len(taps)), t.tobytes(), struct.pack("<i", len(lens)),
                 np.asarray(lens, np.int32).tobytes(), np.asarray(x, np.float32).tobytes()]
    (d / "cases.bin").write_bytes(b"".join(blob))
    out = subprocess.run([exe, str(d / "cases.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("symsync core ok"), out.stdout[-2000:] + out.stderr[-2000:]
    raw = (d / "results.bin").read_bytes()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos)
        pos += a.nbytes
        return a

    res = []
    for _, _, lens, _ in cases:
        per = []
        for _ in lens:
            words = take(np.uint64, int(take(np.int32, 1)[0]))
            k = int(take(np.int32, 1)[0])
            idx, clk, syms = take(np.uint32, k), take(np.float32, k), take(np.float32, k)
            four, sign = take(np.float32, 4), int(take(np.int32, 1)[0])
            hist = take(np.float32, int(take(np.int32, 1)[0]))
            per.append({"words": words, "idx": idx, "clk": clk, "syms": syms,
                        "state": {"clock": four[0], "stream_pos": four[1], "last_sym_boundary_pos": four[2], "next_sym_middle": four[3],
                                  "last_sign": bool(sign), "hist": hist}})
        res.append(per)
    assert pos == len(raw)
    return cases, res


def test_symsync_core_equals_the_model_bit_for_bit(emu):
    """symbols, clock values, indices and the state after EVERY push, for the reference's own test, the three parameter sets of the
    examples, 1 / 2 / 8 taps, pushes of 0, 1, 63, 64, 65 and random lengths, the idle gap and NaN / +-Inf / +-0.0 samples"""
    cases, res = emu
    seen = set()
    for (name, prm, lens, x), per in zip(cases, res):
        m = sm.SymbolSync(*prm)
        pos = 0
        for ln, r in zip(lens, per):
            syms, clk, idx = m.run(x[pos:pos + ln])
            pos += ln
            assert np.array_equal(r["idx"].astype(np.int64), idx), name
            assert sm.bits_equal(r["clk"], clk) and sm.bits_equal(r["syms"], syms), name
            # (a NaN the filter made is compared as a NaN: its payload is the implementation's)
            assert (sm.states_match if name == "non-finite clock" else sm.states_equal)(r["state"], m.state()), name
        seen.add(name)
        if name == "reference test":
            assert per[0]["idx"].tolist() == [2, 6]
        if name == "idle gap":
            # the long `while t > mx` loop (3000 samples at a clock of at most sps + 0.1), then the 3000 samples come off the
            # positions in steps of 10 clock <= 53.1
            assert m.max_fold_iters > 500 and m.step_backs >= 56
        if name == "a gap of 2^18 samples":
            assert m.max_fold_iters > 40000 and m.step_backs > 1000
        if name == "sps 1.25":
            assert sum(len(r["syms"]) for r in per) >= 0.99 * len(x)
        if name == "sps 200":
            assert 10 <= sum(len(r["syms"]) for r in per) <= 20
        if name == "non-finite clock":
            # the first clock update makes the clock NaN: 5 symbols in front of it, none behind
            assert len(per[0]["syms"]) == 5 and m.clock_updates >= 1 and np.isnan(m.state()["clock"])
            assert np.isnan(per[0]["state"]["clock"]) and np.isnan(per[0]["state"]["hist"]).all() and per[0]["idx"].max() < 64
        if name.startswith("adaptive"):
            assert m.clock_updates > 200 and len(set(np.concatenate([r["clk"] for r in per]).view(np.uint32).tolist())) > 100
    assert len(seen) == len(cases)


def test_sign_packing_at_every_word_seam(emu):
    """bit b of word w of a window = x[64 w + b] > 0.0, zeros beyond the window: windows that begin at every position of the
    stream's 64-sample grid, and NaN / +-Inf / +-0.0"""
    cases, res = emu
    starts = set()
    for (name, _, lens, x), per in zip(cases, res):
        pos = 0
        for ln, r in zip(lens, per):
            assert np.array_equal(r["words"], sm.sign_words(x[pos:pos + ln])), name
            if name.startswith("a word seam"):
                starts.add(pos % 64)
            pos += ln
    assert starts == set(range(64))
    w = sm.sign_words(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.0], np.float32))
    assert w.tolist() == [0b10100010]


def test_host_logic_under_the_host_sanitizers(tmp_path):
    """every refusal, the stride edges and hostile counts above n as a stand-alone program built with
    -fsanitize=address,undefined (rustradio_amd/csrc/symsync_host.hpp compiles without HIP)"""
    exe = str(tmp_path / "test_symsync_hostlogic")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "test_symsync_hostlogic.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("symsync host logic ok")


# ---- the library without a device ------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("rr_symbol_sync_create", "rr_symbol_sync_push_dev", "rr_symbol_sync_push", "rr_symbol_sync_produced",
               "rr_symbol_sync_counts_dev", "rr_symbol_sync_dims", "rr_debug_symbol_sync_state")


def test_symbols_are_declared_exported_and_typed():
    from rustradio_amd._lib import SYMBOLS
    L = ctypes.CDLL(rr.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in SYMBOLS and hasattr(L, s)
    assert rr._raw_lib().rr_abi_version() == 3
    T = rr._raw_lib()
    sz, vp, f32, psz = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float, ctypes.POINTER(ctypes.c_size_t)
    for s in NEW_SYMBOLS:
        fn = getattr(T, s)
        assert fn.argtypes is not None and fn.restype in (ctypes.c_int, ctypes.c_void_p), s
    assert T.rr_symbol_sync_create.argtypes == [f32, f32, vp, sz, sz] and T.rr_symbol_sync_create.restype == vp
    assert T.rr_symbol_sync_push_dev.argtypes == [vp, vp, sz, sz, vp, vp, sz, vp]
    assert T.rr_symbol_sync_push.argtypes == [vp, vp, sz, sz, vp, vp, sz, psz]
    assert T.rr_symbol_sync_produced.argtypes == [vp, psz, sz, psz]
    assert T.rr_symbol_sync_counts_dev.argtypes == [vp] and T.rr_symbol_sync_counts_dev.restype == vp
    assert T.rr_symbol_sync_dims.argtypes == [vp, psz]
    assert T.rr_debug_symbol_sync_state.argtypes == [vp, sz, vp, ctypes.POINTER(ctypes.c_int), vp, sz, psz]


@pytest.mark.parametrize("args, sentence", [
    ((1.0, 0.1, [1.0]), "sps must be above 1"),
    ((0.0, 0.1, [1.0]), "sps must be above 1"),
    ((float("nan"), 0.1, [1.0]), "sps must be above 1"),
    ((4.0, -0.01, [1.0]), "max_deviation out of range"),
    ((4.0, 2.01, [1.0]), "max_deviation out of range"),
    ((4.0, float("nan"), [1.0]), "max_deviation out of range"),
    ((4.0, 1.0, []), "SymbolSync needs 1 to 8 finite taps"),
    ((4.0, 1.0, [0.1] * 9), "SymbolSync needs 1 to 8 finite taps"),
    ((4.0, 1.0, [0.5, float("inf")]), "SymbolSync needs 1 to 8 finite taps"),
    ((4.0, 1.0, [float("nan")]), "SymbolSync needs 1 to 8 finite taps"),
    ((4.0, 1.0, [1.0], 0), "nstreams out of range"),
    ((4.0, 1.0, [1.0], 4097), "nstreams out of range"),
])
def test_refusals_come_before_any_device(args, sentence):
    with pytest.raises(ValueError, match=sentence):
        rr.SymbolSync(*args)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        assert rr.SymbolSync(4.0, 1.0, [1.0]).name == "SymbolSync"
    else:
        with pytest.raises(ValueError, match="no usable HIP device"):
            rr.SymbolSync(4.0, 1.0, [1.0], 2)
