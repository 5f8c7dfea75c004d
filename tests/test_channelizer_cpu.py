"""The channelizer's public interface without a GPU: both constructors are declared in the header, bound in the Python
symbol table and in the Rust shim's extern block with matching prototypes, and refuse to run without a HIP device."""
import os
import re

import numpy as np
import pytest

import rustradio_amd as rr
from harness import max_norm_err, resampled_filter_truth, run_chain
from oracle import pyoracle as orc
from rustradio_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rr_channelizer_create", "rr_channelizer_u8_create")


def _header():
    with open(os.path.join(ROOT, "include", "rustradio_amd.h")) as f:
        return f.read()


def _params(decl):
    return [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_constructor(name):
    m = re.search(r"rr_block \*" + name + r"\(([^)]*)\);", _header())
    assert m, name
    assert _params(m.group(1)) == ["const rr_c32 *taps", "size_t nchan", "size_t ntaps", "size_t interp", "size_t deci"]


@pytest.mark.parametrize("name", NAMES)
def test_python_binds_the_constructor(name):
    assert name in _lib.SYMBOLS
    with open(os.path.join(ROOT, "rustradio_amd", "_lib.py")) as f:
        src = f.read()
    assert f"L.{name}.argtypes = [vp, sz, sz, sz, sz]; L.{name}.restype = vp" in src
    assert callable(rr.Channelizer) and callable(rr.ChannelizerU8)


@pytest.mark.parametrize("name", NAMES)
def test_rust_shim_binds_the_constructor(name):
    with open(os.path.join(ROOT, "rust", "src", "lib.rs")) as f:
        src = f.read()
    blk = re.search(r'unsafe extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    m = re.search(r"fn " + name + r"\(([^)]*)\) -> \*mut RrBlock;", blk)
    assert m, name
    assert _params(m.group(1)) == ["taps: *const Complex", "nchan: usize", "ntaps: usize", "interp: usize", "deci: usize"]
    assert "pub struct GpuChannelizer" in src and "impl Block for GpuChannelizer" in src


def test_cpp_mirror_has_the_one_channel_block():
    with open(os.path.join(ROOT, "rustradio_amd", "host", "rustradio.hpp")) as f:
        src = f.read()
    assert re.search(r"inline auto FftFilterResampler\(ReadStream<Complex> src, .*\n.*Fused<Complex, Complex>::make", src)


def test_channelizer_needs_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    taps = np.ones((2, 8), np.complex64)
    with pytest.raises(ValueError, match="no usable HIP device"):
        rr.Channelizer(taps, 1, 5)
    with pytest.raises(ValueError, match="no usable HIP device"):
        rr.ChannelizerU8(taps, 1, 5)


# ---- the oracle chain against the float64 statement of the operation ---------------------------------------------------
ORACLE_MEASURED = 7.11e-7                 # the largest max_norm_err(oracle, truth) over the set below (poly-1535-1:2)
ORACLE_BAR = min(4 * ORACLE_MEASURED, 1e-5 / 4)     # 4 x that is 2.84e-6: held at the cap 1e-5 / 4, 3.5 x the measured value


def _oracle_truth_set():
    """(tag, taps [channels to run][ntaps], I, D, source, the Complex samples the filter sees) of every streaming case of
    tests/test_gpu_channelizer.py and every draw of test_fuzz_channelizer: the first, middle and last channel of each"""
    import test_gpu_channelizer as tc
    import test_gpu_fuzz as tf
    for name, family, L, I, D, nchan, opts, u8 in tc.STREAM_CASES:
        S, cap_in, cap_out, n = tc.stream_plan(L, I, D)
        src, x = tc.stream_source(name, n, nchan, u8)
        yield name, tc.case_taps(L, nchan)[sorted({0, nchan // 2, nchan - 1})], I, D, src, x
    for seed in tf.CHAN_SEEDS:
        d = tf.draw_channelizer(seed)
        x = run_chain([orc.RtlSdrDecode()], d["src"]) if d["u8"] else d["src"]
        yield f"fuzz-{seed}", d["taps"][sorted({0, d["nchan"] // 2, d["nchan"] - 1})], d["I"], d["D"], d["src"], x


def test_oracle_chain_is_the_float64_statement():
    """FftFilter -> RationalResampler of the oracle (pinned so far only by the reference's short known-answer vectors) against
    harness.resampled_filter_truth — y = taps * x in complex128, out[r] = y[(r D) // I], no block and no ring in it — over
    every streaming case of tests/test_gpu_channelizer.py and every draw of test_fuzz_channelizer (first, middle and last
    channel): the same length rule, and max_norm_err(oracle, truth) below the bar.
    Measured over that whole set: between 4.6e-8 (one tap) and 7.10e-7 (poly-1535-1:2; the fuzz draws stay below 3.3e-7).
    4 x the largest is 2.84e-6, which is ABOVE the cap of 1e-5 / 4 = 2.5e-6 the bar has to stay under, so the bar is the
    cap (asserted strictly below it): 3.5 x the measured value instead of 4 x.  The margin covers other seeds; an index or
    block-boundary error in the chain is of order 1.  With it the GPU tests' bound on the distance to the truth,
    1e-5 + max_norm_err(oracle, truth), stays within 1.25e-5."""
    worst, at = 0.0, None
    for tag, taps, I, D, src, x in _oracle_truth_set():
        pre = [orc.RtlSdrDecode()] if src.dtype == np.uint8 else []
        S = orc.fftfilter_dims(orc.FftFilter(taps[0]))[1]
        for t in taps:
            yo = run_chain(pre + [orc.FftFilter(t), orc.RationalResampler(I, D)], src)
            assert len(yo) == -(-(len(x) // S * S) * I // D) > 0, (tag, len(yo))       # whole filter blocks, ceil(n1 I / D)
            e = max_norm_err(yo, resampled_filter_truth(t, x, I, D, len(yo)))
            if e > worst:
                worst, at = e, tag
            assert e < ORACLE_BAR <= 1e-5 / 4, (tag, e)
    print(f"largest max_norm_err(oracle, truth) = {worst:.3g} at {at}")


def test_stream_plans_meet_their_conditions_under_the_model():
    """the windows tests/test_gpu_channelizer.py drives every streaming case with, run through the protocol models alone: odd
    windows, cap_out of at least one block, four emitting calls or more, a WAIT_DST, a.A of both parities where the filter
    block is odd — and the path the constructor's rules give is the one the case is listed under"""
    import test_gpu_channelizer as tc
    for name, family, L, I, D, nchan, opts, u8 in tc.STREAM_CASES:
        assert tc.expected_kernel(L, I, D, opts) == family, name
        S, cap_in, cap_out, n = tc.stream_plan(L, I, D)
        src, _ = tc.stream_source(name, n, 1, u8) if family == "per channel" else (np.zeros(2 * n + 1 if u8 else n, np.uint8 if u8 else np.complex64), None)
        cin = (2 * cap_in) | 1 if u8 else cap_in
        taps0 = tc.case_taps(L, nchan)[0]
        _, log = tc.ring_calls(lambda calls: tc.expected_log(family, taps0, I, D, src, calls), len(src), cin, cap_out)
        tc.assert_stream_conditions(name, family, S, I, D, cin, cap_out, log, u8)
