"""No GPU: the sequential models of tests/saver_model.py against the reference's own Delay vectors and against the closed form
of StreamToPdu on the delayed stream, the host-only logic of Delay and the burst saver under the host sanitizers, and what the
new create calls refuse without a device."""
import os
import subprocess

import numpy as np
import pytest

import burst_model as bm
import pdu_model as pm
import rustradio_amd as rr
import saver_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the reference's own vectors (src/delay.rs, mod tests) -----------------------------------------------------------------------------
def test_delay_zero_and_delay_one():
    (st, c, p, need, out), = sm.delay_model([[1.0, 2.0, 3.0]], 0, [1000])
    assert out == [1.0, 2.0, 3.0] and (st, c, p, need) == (sm.WAIT_SRC, 3, 3, 1)
    (st, c, p, need, out), = sm.delay_model([[1.0, 2.0, 3.0]], 1, [1000])
    assert out == [0, 1.0, 2.0, 3.0] and (st, c, p, need) == (sm.WAIT_SRC, 3, 4, 1)


def test_eof_waits_for_pending_delay():
    """model only: the reference's stream holds 1,024,000 u32, so the delay of its test is 1,024,001 — above the device cap"""
    cap = 4_096_000 // 4
    m = sm.DelaySeq(cap + 1)
    assert not m.eof(True)
    st, c, p, need, out = m.work(cap)
    assert (st, c, p, need) == (sm.WAIT_DST, 0, cap, 1) and not any(out)
    assert not m.eof(True)
    st, c, p, need, out = m.work(cap)                 # the reader has consumed the stream: cap free elements again
    assert (st, c, p, need) == (sm.WAIT_SRC, 0, 1, 1) and out == [0]
    assert m.eof(True) and not m.eof(False)


def test_delay_model_return_points():
    # no output space: WAIT_DST whatever else holds (delay.rs:79-82 comes before the input test)
    assert sm.delay_model([[1, 2]], 3, [0]) == [(sm.WAIT_DST, 0, 0, 1, [])]
    assert sm.delay_model([[]], 0, [0]) == [(sm.WAIT_DST, 0, 0, 1, [])]
    # several calls that emit only zeros, then one that ends inside the copy, then the rest
    res = sm.delay_model([[1, 2, 3]] * 3 + [[3]], 5, [2, 2, 3, 9])
    assert res == [(sm.WAIT_DST, 0, 2, 1, [0, 0]), (sm.WAIT_DST, 0, 2, 1, [0, 0]), (sm.WAIT_DST, 2, 3, 1, [0, 1, 2]),
                   (sm.WAIT_SRC, 1, 1, 1, [3])]
    assert sm.delayed([1, 2, 3, 4], 2) == [0, 0, 1, 2] and sm.delayed([1, 2], 5) == [0, 0]


# ---- the saver model against the closed form on the delayed stream ---------------------------------------------------------------------
def plain(per):
    return [[(f, [complex(v) for v in p]) for f, p in w] for w in per]


def test_saver_model_equals_the_closed_form_on_the_delayed_stream():
    """delay 0..12, tail 0..5, max_size 0..12, up to three cuts, cuts shorter than the delay among them"""
    rng = np.random.default_rng(11)
    npdus = short = zeros = 0
    for _ in range(3000):
        n = int(rng.integers(1, 48))
        amp = np.repeat(rng.random(n // 3 + 1) < rng.choice([0.2, 0.5, 0.8]), 3)[:n]
        x = ((amp * 1.0 + 0.001) * np.exp(1j * np.arange(n))).astype(np.complex64)
        delay, ms, tl = int(rng.integers(0, 13)), int(rng.integers(0, 13)), int(rng.integers(0, 6))
        sp = sorted(set(int(v) for v in rng.integers(0, n + 1, int(rng.integers(0, 4)))))
        cuts = [0] + sp + [n]
        short += any(0 < b - a < delay for a, b in zip(cuts[:-1], cuts[1:]))
        m = sm.SaverSeq(0.5, 0.25, delay, ms, tl)
        got = [m.push(x[a:b])[0] for a, b in zip(cuts[:-1], cuts[1:])]
        env, _ = bm.iir_ref_f32(bm.mag2_f32(x), 0.5)
        d = np.array(sm.delayed(x, delay, np.complex64(0)), np.complex64)
        want = pm.closed_form_windows(d, env, 0.25, ms, tl, sp)
        assert plain(got) == plain(want), (n, delay, ms, tl, sp)
        npdus += sum(len(w) for w in got)
        zeros += sum(1 for w in got for f, p in w if f is not None and f < delay)
    assert npdus > 1000 and short > 300 and zeros > 50, (npdus, short, zeros)


# ---- the host-only logic ---------------------------------------------------------------------------------------------------------------
def test_host_logic_under_the_host_sanitizers(tmp_path):
    """the refusals, one work() of Delay against a loop written out, the history plan against a simulation of many short pushes
    and the launch count, as a stand-alone program built with -fsanitize=address,undefined (saver_host.hpp compiles without HIP)"""
    exe = str(tmp_path / "test_saver_hostlogic")
    src = os.path.join(ROOT, "tests", "cpp", "test_saver_hostlogic.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("saver host logic ok")


# ---- what is refused before any device is touched ---------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    n0 = rr.lib().rr_debug_kernel_launches()
    for es in (0, 2, 3, 16):
        assert not rr.lib().rr_delay_create(5, es) and rr.last_error() == "unsupported element size"
    assert not rr.lib().rr_delay_create(1_024_001, 4) and rr.last_error() == "delay: more than 1,024,000 samples"
    assert not rr.lib().rr_stream_to_pdu_c32_create(0.5, 512_001, 0) and rr.last_error() == "max_size beyond 512000 samples"
    for alpha in (-0.1, 1.5, float("nan")):
        assert not rr.lib().rr_burst_saver_create(alpha, 0.5, 10, 10, 1) and rr.last_error() == "alpha out of range"
    assert not rr.lib().rr_burst_saver_create(0.1, 0.5, 10, 512_001, 1) and rr.last_error() == "max_size beyond 512000 samples"
    assert not rr.lib().rr_burst_saver_create(0.1, 0.5, 1_024_001, 10, 1) and rr.last_error() == "delay: more than 1,024,000 samples"
    with pytest.raises(ValueError, match="unsupported element size"):
        rr.Delay(3, np.complex128)
    with pytest.raises(ValueError, match="alpha out of range"):
        rr.BurstSaver(2.0, 0.5, 10, 10, 1)
    assert rr.lib().rr_burst_saver_push_dev(None, None, 4, None, None) != 0 and "not a burst saver handle" in rr.last_error()
    assert rr.lib().rr_burst_saver_dims(None, 4, None, None) != 0 and "not a burst saver handle" in rr.last_error()
    assert rr.lib().rr_pdu_fetch_c32(None, 0, None, 0) != 0 and "not a stream_to_pdu handle" in rr.last_error()
    assert rr.lib().rr_debug_kernel_launches() == n0


def test_symbols():
    from rustradio_amd._lib import SYMBOLS
    for s in ("rr_delay_create", "rr_stream_to_pdu_c32_create", "rr_stream_to_pdu_push_c32", "rr_pdu_fetch_c32", "rr_burst_saver_create",
              "rr_burst_saver_push_dev", "rr_burst_saver_push", "rr_burst_saver_dims"):
        assert s in SYMBOLS and hasattr(rr.lib(), s)
    assert rr.TAGS_SHIFT == 3 and rr.lib().rr_abi_version() == 3
