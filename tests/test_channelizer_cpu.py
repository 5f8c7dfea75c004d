"""The channelizer's public interface without a GPU: both constructors are declared in the header, bound in the Python
symbol table and in the Rust shim's extern block with matching prototypes, and refuse to run without a HIP device."""
import os
import re

import numpy as np
import pytest

import rustradio_amd as rr
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
