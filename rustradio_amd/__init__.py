"""rustradio_amd — MI355X-native implementation of rustradio's streaming-DSP hot path.

Host-side mirror (Python, over the C ABI of include/rustradio_amd.h) of the reference's
block interface for this path: the constructors take what `X::new(src, ...)` / the
builders take (minus the stream, which the caller owns), and `work()` is
`Block::work()` over explicit stream windows, returning the BlockRet variant plus
what the reference would pass to `consume()`/`produce()`.

    FirFilter            src/fir.rs:303-551      (builder: taps, .deci(), .translate())
    FftFilter            src/fft_filter.rs:210-355
    FftFilterFloat       src/fft_filter.rs:365-491
    RationalResampler    src/rational_resampler.rs:100-213
    QuadratureDemod      src/quadrature_demod.rs:32-114
    RtlSdrDecode         src/rtlsdr_decode.rs:9-47
    Hilbert              src/hilbert.rs:22-129
    Wpcr                 src/wpcr.rs:84-239      (message form: a batch of bursts per call)
    StreamToPdu          src/burst_tagger.rs:68-85, src/stream_to_pdu.rs:198-275, src/wpcr.rs:44-82 (BurstTagger -> StreamToPdu -> Midpointer)
    SymbolSync           src/symbol_sync.rs:46-217, src/iir_filter.rs:104-125   (N streams per handle, a window of each per call)
    AddConst             src/add_const.rs:51-68
    AfskDemod            Hilbert -> QuadratureDemod -> FftFilterFloat -> AddConst, examples/ax25-1200-rx.rs:238-247 (N streams per handle)
    AmDemod              norm -> FftFilterFloat -> RationalResampler -> MultiplyConst, examples/airspy_am_decode.rs (N streams per handle)
    AirspyDecode         examples/airspy_am_decode.rs, the Map "AirSPY to Complex"
    FskTx                line bits -> AFSK / FSK baseband, examples/bell202.rs:166-183, examples/g3ruh.rs:256-272 (a push of bits per call)
    low_pass / low_pass_complex / hilbert_taps / make_window   src/fir.rs:594-680, src/window.rs

All sample arithmetic runs in HIP kernels on the GPU; nothing here computes samples.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import contextlib
import math
import struct
import threading

from ._lib import BuildOpts, lib as _raw_lib, last_error, LIB_PATH  # noqa: F401

# BlockRet (src/block.rs:12-70)
AGAIN, WAIT_SRC, WAIT_DST, EOF, PENDING, ERR = 0, 1, 2, 3, 4, -1
# WindowType (src/window.rs:42-60)
WIN_HAMMING, WIN_BLACKMAN, WIN_BLACKMAN_HARRIS, WIN_HAMMING_PARM = 0, 1, 2, 3
ATAN2_EXACT, ATAN2_FAST = 0, 1
ROT_MODEL, ROT_REPLAY, ROT_REPLAY_DEVICE, ROT_REPLAY_HOST = 0, 1, 2, 3
DEMOD_FASTFM = 2        # fused-chain constructors: FastFM in the demodulator's place (RR_DEMOD_FASTFM)
DEFAULT_STREAM_SIZE = 4_096_000  # bytes, src/stream.rs:105


# ---- per-block path overrides (rr_build_opts) ---------------------------------------------
# `build_options(...)` is a context manager: every block / DeviceStream created inside it is built with these
# overrides (each create call gets its own rr_next_create_options; nothing is read from the environment).
PATH_AUTO, PATH_DIRECT, PATH_FFT = 0, 1, 2
_build_opts: dict = {}                 # process-wide defaults (tests patch this through harness.knob)
_tls = threading.local()               # build_options() is per THREAD, like the C side's pending overrides
_PATHS = {"auto": PATH_AUTO, "direct": PATH_DIRECT, "fft": PATH_FFT}
# the create calls that CONSUME rr_next_create_options (abi.cpp OptsScope): every block constructor and rr_dstream_create.
# rr_fanout_create does not — handing it the overrides would leave them pending for the thread's next block
_NO_OPTS_CREATES = ("rr_fanout_create",)


def _effective_opts() -> dict:
    o = getattr(_tls, "opts", None)
    return _build_opts if o is None else o


@contextlib.contextmanager
def build_options(**kw):
    """fir_path='direct'|'fft', fir_prune=+-1, fir_half=-1, fir_cfg=0..7, fft_log2f=10..14, fft_no_split=1,
    fftfloat_complex=1, fm_full=1, fm_poly=-1 (8 / 12: the multi-channel kernel variant), dstream_no_vmm=1, fir_poly=+-1,
    fft_nonfinite_tiles=1 (none) | 3 (in the tile kernel's tail), host_in_staged=+-1, sync_lanes=1 | 64 (SymbolSync: streams
    per wave of the clock kernel), sync_prof_launch=1..3 (SymbolSync: profile() times that launch alone)"""
    prev = getattr(_tls, "opts", None)
    _tls.opts = dict(_effective_opts(), **kw)
    try:
        yield
    finally:
        _tls.opts = prev


class _CreateProxy:
    """the loaded library; rr_*_create / rr_dstream_create first hand the pending overrides to the C ABI"""

    def __getattr__(self, name):
        f = getattr(_raw_lib(), name)
        opts = _effective_opts()
        if not (name.endswith("_create") and name not in _NO_OPTS_CREATES and opts):
            return f

        def create(*a):
            o = BuildOpts()
            for k, v in opts.items():
                if k == "fir_path":
                    v = _PATHS.get(v, v)
                if k == "fir_cfg":
                    k, v = "fir_cfg_plus1", int(v) + 1
                setattr(o, k, int(v))
            if _raw_lib().rr_next_create_options(C.byref(o)) != 0:
                raise ValueError(last_error())
            return f(*a)
        return create


_proxy = _CreateProxy()


def lib():
    return _proxy


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _fetch(fn, handle, *dtypes, tail=()):
    """ask for the total, allocate, ask again: fn(handle, one array per dtype, capacity, &total, *tail) -> the arrays, cut to total"""
    total = C.c_size_t(0)
    if fn(handle, *[None] * len(dtypes), 0, C.byref(total), *tail) != 0:
        raise RuntimeError(last_error())
    arrs = [np.zeros(max(total.value, 1), d) for d in dtypes]
    if total.value and fn(handle, *map(_ptr, arrs), total.value, C.byref(total), *tail) != 0:
        raise RuntimeError(last_error())
    return [a[:total.value] for a in arrs]


def device_count() -> int:
    return lib().rr_device_count()


def set_device(ordinal: int) -> None:
    if lib().rr_set_device(ordinal) != 0:
        raise ValueError(last_error())


# ---- tap designers --------------------------------------------------------------------
def make_window(wtype: int, ntaps: int, parm: float = 0.0) -> np.ndarray:
    out = np.zeros(ntaps, np.float32)
    if lib().rr_make_window(wtype, parm, ntaps, _ptr(out)) != 0:
        raise ValueError(last_error())
    return out


def compute_ntaps(samp_rate, twidth, wtype=WIN_HAMMING) -> int:
    return lib().rr_compute_ntaps(samp_rate, twidth, wtype)


def low_pass(samp_rate, cutoff, twidth, wtype=WIN_HAMMING, parm=0.0) -> np.ndarray:
    n = lib().rr_low_pass(samp_rate, cutoff, twidth, wtype, parm, None, 0)
    if n == 0:
        raise ValueError(last_error())
    out = np.zeros(n, np.float32)
    lib().rr_low_pass(samp_rate, cutoff, twidth, wtype, parm, _ptr(out), n)
    return out


def low_pass_complex(samp_rate, cutoff, twidth, wtype=WIN_HAMMING, parm=0.0) -> np.ndarray:
    n = lib().rr_low_pass_complex(samp_rate, cutoff, twidth, wtype, parm, None, 0)
    if n == 0:
        raise ValueError(last_error())
    out = np.zeros(n, np.complex64)
    lib().rr_low_pass_complex(samp_rate, cutoff, twidth, wtype, parm, _ptr(out), n)
    return out


def multiband(bands, window):
    """fir::multiband(bands, taps, window) (src/fir.rs:552-590) -> complex64 taps, or None (the reference's None)"""
    b = np.ascontiguousarray(bands, np.float32).reshape(-1, 2)
    w = np.ascontiguousarray(window, np.float32)
    out = np.zeros(len(w), np.complex64)
    return out if lib().rr_multiband(_ptr(b), len(b), _ptr(w), len(w), _ptr(out)) == 0 else None


def hilbert_taps(window: np.ndarray) -> np.ndarray:
    w = np.ascontiguousarray(window, np.float32)
    out = np.zeros(len(w), np.float32)
    if lib().rr_hilbert_taps(_ptr(w), len(w), _ptr(out)) != 0:
        raise ValueError(last_error())
    return out


# ---- blocks ---------------------------------------------------------------------------
class Block:
    """One block instance (an opaque `rr_block`)."""

    def __init__(self, handle, in_dtype, out_dtype):
        if not handle:
            raise ValueError(last_error())
        self._h = handle
        self.in_dtype = np.dtype(in_dtype)
        self.out_dtype = np.dtype(out_dtype)
        assert lib().rr_block_in_elem_size(handle) == self.in_dtype.itemsize
        assert lib().rr_block_out_elem_size(handle) == self.out_dtype.itemsize

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().rr_block_destroy(h)
            except Exception:
                pass

    @property
    def name(self) -> str:
        """BlockName::block_name (src/block.rs:91-97)."""
        return lib().rr_block_name(self._h).decode()

    def work(self, inp: np.ndarray, out_cap: int):
        """Block::work() over host windows -> (status, consumed, produced, need, out[:produced])."""
        inp = np.ascontiguousarray(inp, self.in_dtype)
        nw = lib().rr_block_out_windows(self._h)
        out = np.zeros(max(out_cap, 1) * nw, self.out_dtype)
        c, p, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        st = lib().rr_block_work(self._h, _ptr(inp), len(inp), _ptr(out), out_cap,
                                 C.byref(c), C.byref(p), C.byref(n))
        if st == ERR:
            raise RuntimeError(last_error())
        if nw > 1:      # multi-output block: (windows, produced)
            return st, c.value, p.value, n.value, out.reshape(nw, max(out_cap, 1))[:, :p.value].copy()
        return st, c.value, p.value, n.value, out[:p.value]

    def work_into(self, inp: np.ndarray, out: np.ndarray, out_cap: int):
        """Block::work() over caller-owned host windows (no allocation, no copy on the Python side): exactly the
        call the Rust shim makes with read_buf() / write_buf() slices -> (status, consumed, produced, need)"""
        assert inp.dtype == self.in_dtype and out.dtype == self.out_dtype and inp.flags.c_contiguous and out.flags.c_contiguous
        assert len(out) >= out_cap * lib().rr_block_out_windows(self._h)
        c, p, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        st = lib().rr_block_work(self._h, _ptr(inp), len(inp), _ptr(out), out_cap, C.byref(c), C.byref(p), C.byref(n))
        if st == ERR:
            raise RuntimeError(last_error())
        return st, c.value, p.value, n.value

    def work_dev(self, d_in: int, in_len: int, d_out: int, out_cap: int, stream: int = 0):
        """Block::work() over DEVICE windows (raw device pointers, e.g. tensor.data_ptr());
        asynchronous on `stream` (a hipStream_t handle used as given; 0 = the default stream, which is
        what torch.cuda.current_stream().cuda_stream returns for torch's default stream)
        -> (status, consumed, produced, need)."""
        c, p, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        st = lib().rr_block_work_dev(self._h, C.c_void_p(d_in), in_len, C.c_void_p(d_out), out_cap,
                                     C.byref(c), C.byref(p), C.byref(n), C.c_void_p(stream))
        if st == ERR:
            raise RuntimeError(last_error())
        return st, c.value, p.value, n.value

    def work_streams(self, src: "DeviceStream", dst: "DeviceStream", stream: int = 0):
        """Block::work() between two device-resident streams (windows, consume and produce handled by the
        library) -> (status, consumed, produced, need); asynchronous on `stream`."""
        c, p, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        st = lib().rr_block_work_streams(self._h, src._h, dst._h, C.byref(c), C.byref(p), C.byref(n), C.c_void_p(stream))
        if st == ERR:
            raise RuntimeError(last_error())
        return st, c.value, p.value, n.value

    def eof(self, src_eof: bool) -> bool:
        """BlockEOF::eof (src/block.rs:103-110)."""
        return bool(lib().rr_block_eof(self._h, int(src_eof)))

    def set_rotator_mode(self, mode: int) -> None:
        """rr_fir_set_rotator_mode on a translating FirFilter / HilbertFir: ROT_REPLAY (default, the reference's recurrence) or ROT_MODEL"""
        if lib().rr_fir_set_rotator_mode(self._h, mode) != 0:
            raise ValueError(last_error())

    def sync(self) -> None:
        if lib().rr_block_sync(self._h) != 0:
            raise RuntimeError(last_error())

    def last_kernel(self) -> str:
        """rr_debug_last_kernel: the kernel family of the most recent emitting work() call ("" for a block without a per-call
        choice or before the first output) — introspection for tests"""
        return lib().rr_debug_last_kernel(self._h).decode()

    def set_profiling(self, on: bool) -> None:
        lib().rr_block_set_profiling(self._h, int(on))

    def profile(self, reset: bool = True):
        """-> (summed dominant-kernel time in ms, launches), from HIP events on the launch stream."""
        ms, n = C.c_double(0), C.c_size_t(0)
        if lib().rr_block_profile(self._h, C.byref(ms), C.byref(n), int(reset)) != 0:
            raise RuntimeError(last_error())
        return ms.value, n.value


def host_ring(nbytes: int) -> np.ndarray:
    """a page-aligned, whole-pages host buffer (one private anonymous mapping, like the reference's ring:
    src/nowasm/circular_buffer.rs:98-128) as a uint8 array of at least `nbytes` — the only kind of range rr_host_register
    grants zero-copy windows on (include/rustradio_amd.h)"""
    import mmap
    size = -(-max(int(nbytes), 1) // mmap.PAGESIZE) * mmap.PAGESIZE
    return np.frombuffer(mmap.mmap(-1, size), dtype=np.uint8)


def host_register(a: np.ndarray) -> None:
    """page-lock a host array that will be handed to work()/push()/pop() (rr_host_register)"""
    if lib().rr_host_register(_ptr(a), a.nbytes) != 0:
        raise RuntimeError(last_error())


def host_window_in_place(a: np.ndarray) -> bool:
    """whether work_into() lets the kernels read / write this host window in place (rr_host_window_in_place)"""
    return bool(lib().rr_host_window_in_place(_ptr(a), a.nbytes))


def host_unregister(a: np.ndarray) -> None:
    if lib().rr_host_unregister(_ptr(a)) != 0:
        raise RuntimeError(last_error())


class DeviceStream:
    """new_stream() (src/stream.rs:336-339) in HBM: rr_dstream.  Same window contract as ReadStream /
    WriteStream: everything readable / all free space, contiguous; `capacity_bytes` as the reference's
    DEFAULT_STREAM_SIZE."""

    def __init__(self, dtype, capacity_bytes: int = 4_096_000):
        self.dtype = np.dtype(dtype)
        self._h = lib().rr_dstream_create(self.dtype.itemsize, capacity_bytes)
        if not self._h:
            raise RuntimeError(last_error())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().rr_dstream_destroy(h)

    @property
    def capacity(self) -> int:
        return lib().rr_dstream_capacity(self._h)

    @property
    def double_mapped(self) -> bool:
        """True when the ring is one physical allocation mapped twice (no data movement, ever)"""
        return bool(lib().rr_dstream_is_double_mapped(self._h))

    def readable(self) -> int:
        return lib().rr_dstream_read_buf(self._h, None)

    def free(self, stream: int = 0) -> int:
        return lib().rr_dstream_write_buf(self._h, None, C.c_void_p(stream))

    SIDE_WRITER, SIDE_READER = 0, 1

    def close(self, side: int) -> None:
        """drop of the WriteStream / ReadStream end (rr_dstream_close): what the other end's closed() / eof() / wait() see"""
        if lib().rr_dstream_close(self._h, side) != 0:
            raise RuntimeError(last_error())

    def closed(self, side: int) -> bool:
        return bool(lib().rr_dstream_closed(self._h, side))

    def wait(self, side: int, need: int, timeout_ms: int = 100):
        """StreamWait::wait(need) of the `side` end (src/stream.rs:121-126) -> (count seen, never)"""
        never = C.c_int(0)
        n = lib().rr_dstream_wait(self._h, side, need, timeout_ms, C.byref(never))
        return n, bool(never.value)

    def push(self, x: np.ndarray, stream: int = 0) -> int:
        """fill_from_slice + produce of as much of the host array `x` as fits -> elements taken"""
        x = np.ascontiguousarray(x, self.dtype)
        n = min(len(x), self.free(stream))
        if n and (lib().rr_dstream_copy_in(self._h, 0, _ptr(x), n, C.c_void_p(stream)) != 0
                  or lib().rr_dstream_produce(self._h, n) != 0):
            raise RuntimeError(last_error())
        return n

    def produce_resident(self, stream: int = 0) -> int:
        """a device-resident source: everything free becomes readable as it stands in the ring (write_buf + produce, no copy) -> n"""
        n = self.free(stream)
        if n and lib().rr_dstream_produce(self._h, n) != 0:
            raise RuntimeError(last_error())
        return n

    def discard(self) -> int:
        """consume everything readable without copying it anywhere (NullSink, src/null_sink.rs:15-25)"""
        n = self.readable()
        if n and lib().rr_dstream_consume(self._h, n) != 0:
            raise RuntimeError(last_error())
        return n

    def pop(self, n: int = None, stream: int = 0) -> np.ndarray:
        """copy the first n readable elements (default all) to the host and consume them"""
        m = self.readable()
        n = m if n is None else min(n, m)
        out = np.empty(n, self.dtype)
        if n and (lib().rr_dstream_copy_out(self._h, 0, _ptr(out), n, C.c_void_p(stream)) != 0
                  or lib().rr_dstream_consume(self._h, n) != 0):
            raise RuntimeError(last_error())
        return out


FANOUT_TIMING, FANOUT_RCCL_ALWAYS, FANOUT_MESH, FANOUT_ID_BYTES = 1, 2, 4, 128


def fanout_unique_id() -> bytes:
    """rr_fanout_unique_id: the 128-byte group id, made on the owning rank and shipped to the others"""
    buf = C.create_string_buffer(FANOUT_ID_BYTES)
    if lib().rr_fanout_unique_id(buf) != 0:
        raise RuntimeError(last_error())
    return buf.raw


class Fanout:
    """rr_fanout (include/rustradio_amd.h): the double-buffered streaming fan-out of a shared source across GPUs, one
    process per GPU, broadcast over RCCL on a communication stream (replaces the reference's in-process Tee tree,
    src/tee.rs:10-24).  Streams are raw HIP stream handles (0 = the default stream)."""

    def __init__(self, group_id, rank: int, world: int, tile_bytes: int, src_rank: int = 0, flags: int = 0):
        self.rank, self.world, self.src, self.tile_bytes = rank, world, src_rank, tile_bytes
        self._h = lib().rr_fanout_create(group_id, rank, world, src_rank, tile_bytes, flags)
        if not self._h:
            raise RuntimeError(last_error())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:                            # (module globals are gone at interpreter shutdown)
            lib().rr_fanout_destroy(h)

    def produce_buf(self, t: int, stream: int = 0) -> int:
        p = lib().rr_fanout_produce_buf(self._h, t, C.c_void_p(stream))
        if not p:
            raise RuntimeError(last_error())
        return p

    def submit(self, t: int, stream: int = 0) -> None:
        if lib().rr_fanout_submit(self._h, t, C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def acquire(self, t: int, stream: int = 0) -> int:
        p = lib().rr_fanout_acquire(self._h, t, C.c_void_p(stream))
        if not p:
            raise RuntimeError(last_error())
        return p

    def release(self, t: int, stream: int = 0) -> None:
        if lib().rr_fanout_release(self._h, t, C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def stats(self):
        """-> (summed broadcast ms, broadcasts timed) since the last call (FANOUT_TIMING)"""
        ms, n = C.c_double(0), C.c_size_t(0)
        if lib().rr_fanout_stats(self._h, C.byref(ms), C.byref(n)) != 0:
            raise RuntimeError(last_error())
        return ms.value, n.value


def FirFilter(taps, deci: int = 1, translate=None, rotator: int = ROT_REPLAY) -> Block:
    """FirFilter::builder(taps).deci(deci).translate(samp_rate, freq).build(src)."""
    if np.iscomplexobj(np.asarray(taps)):
        t = np.ascontiguousarray(taps, np.complex64)
        fs, f = translate if translate is not None else (0.0, 0.0)
        h = lib().rr_fir_c32_create(_ptr(t), len(t), deci, 1 if translate is not None else 0, fs, f)
        b = Block(h, np.complex64, np.complex64)
        if translate is not None and lib().rr_fir_set_rotator_mode(b._h, rotator) != 0:
            raise ValueError(last_error())
        return b
    if translate is not None:
        raise ValueError("FirFilter asked to translate on non-Complex")  # fir.rs:401
    t = np.ascontiguousarray(taps, np.float32)
    return Block(lib().rr_fir_f32_create(_ptr(t), len(t), deci), np.float32, np.float32)


def FftFilter(taps) -> Block:
    t = np.ascontiguousarray(taps, np.complex64)
    return Block(lib().rr_fftfilter_create(_ptr(t), len(t)), np.complex64, np.complex64)


def FftFilterFloat(taps) -> Block:
    t = np.ascontiguousarray(taps, np.float32)
    return Block(lib().rr_fftfilter_float_create(_ptr(t), len(t)), np.float32, np.float32)


def fftfilter_dims(block: Block):
    """-> (reference fft_size, reference nsamples, GPU tile size)."""
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    if lib().rr_fftfilter_dims(block._h, C.byref(a), C.byref(b), C.byref(c)) != 0:
        raise ValueError(last_error())
    return a.value, b.value, c.value


def fir_uses_fft_tiles(block: Block) -> bool:
    """True when a FirFilter<Complex> runs on overlap-save FFT tiles (deci 1, more than a few taps)."""
    return lib().rr_fir_fft_tile(block._h) != 0


def RationalResampler(interp: int, deci: int, dtype=np.complex64) -> Block:
    dt = np.dtype(dtype)
    return Block(lib().rr_resampler_create(interp, deci, dt.itemsize), dt, dt)


def MultiplyConst(val, dtype=np.float32) -> Block:
    """MultiplyConst::new(src, val) (src/multiply_const.rs:6-23), Float or Complex."""
    if np.dtype(dtype) == np.complex64:
        v = complex(val)
        return Block(lib().rr_multiply_const_c32_create(v.real, v.imag), np.complex64, np.complex64)
    return Block(lib().rr_multiply_const_f32_create(float(val)), np.float32, np.float32)


def AddConst(val, dtype=np.float32) -> Block:
    """AddConst::new(src, val) (src/add_const.rs:51-68), Float or Complex: one f32 add per component, bit-exact."""
    if np.dtype(dtype) == np.complex64:
        v = complex(val)
        return Block(lib().rr_add_const_c32_create(v.real, v.imag), np.complex64, np.complex64)
    return Block(lib().rr_add_const_f32_create(float(val)), np.float32, np.float32)


def FastFM() -> Block:
    """FastFM::new(src) (src/quadrature_demod.rs:144-165)."""
    return Block(lib().rr_fastfm_create(), np.complex64, np.float32)


def FftStream(size: int) -> Block:
    """FftStream::new(src, size) (src/fft_stream.rs:40-117); any size from 2 to the stream capacity (512,000)."""
    h = lib().rr_fftstream_create(size)
    if not h:
        raise ValueError(last_error())
    return Block(h, np.complex64, np.complex64)


class Fft:
    """Fft::from_fft_size(prev, size) (src/fft.rs:19-56): the message (PDU) form of the forward FFT —
    `process(msg)` takes one array of exactly `size` Complex samples and returns its transform."""

    def __init__(self, size: int):
        if size == 0:
            raise ValueError("FFT called with size 0")                    # fft.rs:24-26
        self.size = size
        self._blk = FftStream(size)

    def process(self, msg) -> np.ndarray:
        m = np.ascontiguousarray(msg, np.complex64)
        out = np.empty(len(m), np.complex64) if len(m) else np.empty(1, np.complex64)
        if lib().rr_fft_process(self._blk._h, _ptr(m), len(m), _ptr(out)) != 0:
            raise ValueError(last_error())
        return out[:len(m)]


def RtlSdrDecode() -> Block:
    """RtlSdrDecode::new(src) (src/rtlsdr_decode.rs:9-47): u8 I/Q pairs -> Complex."""
    return Block(lib().rr_rtlsdr_decode_create(), np.uint8, np.complex64)


def QuadratureDemod(gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    return Block(lib().rr_quaddemod_create(gain, mode), np.complex64, np.float32)


def FmChain(taps, interp: int, deci: int, gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    """FftFilter(taps) -> RationalResampler(interp, deci) -> QuadratureDemod(gain) fused into one
    block / one kernel (examples/rtl_fm.rs:381-419 wiring); Complex in, f32 out."""
    t = np.ascontiguousarray(taps, np.complex64)
    return Block(lib().rr_fm_chain_create(_ptr(t), len(t), interp, deci, gain, mode), np.complex64, np.float32)


def FirFftFilter(fir_taps, fft_taps) -> Block:
    """FirFilter<Complex>(fir_taps) -> FftFilter(fft_taps) fused into one convolution with the composite taps
    (rr_fir_fftfilter_create); whole-stream output == the two blocks, incl. FftFilter's zero-history start."""
    t1 = np.ascontiguousarray(fir_taps, np.complex64)
    t2 = np.ascontiguousarray(fft_taps, np.complex64)
    return Block(lib().rr_fir_fftfilter_create(_ptr(t1), len(t1), _ptr(t2), len(t2)), np.complex64, np.complex64)


def FirFmChain(fir_taps, fft_taps, interp: int, deci: int, gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    """FirFilter(fir_taps) -> FftFilter(fft_taps) -> RationalResampler(interp, deci) -> QuadratureDemod(gain) as one
    kernel (rr_fir_fm_chain_create): the metric's whole chain; Complex in, f32 out."""
    t1 = np.ascontiguousarray(fir_taps, np.complex64)
    t2 = np.ascontiguousarray(fft_taps, np.complex64)
    return Block(lib().rr_fir_fm_chain_create(_ptr(t1), len(t1), _ptr(t2), len(t2), interp, deci, gain, mode),
                 np.complex64, np.float32)


def AudioChain(taps, interp: int, deci: int, scale: float = 1.0) -> Block:
    """FftFilterFloat(taps) -> RationalResampler(interp, deci) -> MultiplyConst(scale) fused into one real-valued kernel
    (rr_audio_chain_create; the audio stage of examples/rtl_fm.rs:398-418); f32 in, f32 out."""
    t = np.ascontiguousarray(taps, np.float32)
    return Block(lib().rr_audio_chain_create(_ptr(t), len(t), interp, deci, scale), np.float32, np.float32)


def _f64_bits(k: float) -> int:
    """f64::to_bits: how a double crosses the C ABI exactly (rr_vco_create)"""
    return struct.unpack("<Q", struct.pack("<d", k))[0]


def Vco(k: float) -> Block:
    """Vco::new(src, k) (src/vco.rs:9-37): f32 in, Complex(sin phase, cos phase) out, phase += k * a in f64."""
    return Block(lib().rr_vco_create(_f64_bits(k)), np.float32, np.complex64)


def FmTx(interp: int, deci: int, k: float) -> Block:
    """RationalResampler(interp, deci) -> Vco(k) fused into one block (rr_fm_tx_create; the modulator of
    examples/fm_tx.rs:84-91); f32 in, Complex out."""
    return Block(lib().rr_fm_tx_create(interp, deci, _f64_bits(k)), np.float32, np.complex64)


def AirspyDecode() -> Block:
    """The first Map of examples/airspy_am_decode.rs: AirSPY u32 words (i16 I low, i16 Q high) in, Complex(i / 1000, q / 1000)
    out, bit-exact; windows count u32 elements."""
    return Block(lib().rr_airspy_decode_create(), np.uint32, np.complex64)


def ComplexToMag2() -> Block:
    """ComplexToMag2::new(src) (src/complex_to_mag2.rs:8-21): Complex in, re * re + im * im out, bit-exact."""
    return Block(lib().rr_complex_to_mag2_create(), np.complex64, np.float32)


def SinglePoleIirFilter(alpha: float, dtype=np.float32) -> Block:
    """SinglePoleIirFilter::new(src, alpha) (src/single_pole_iir_filter.rs:11-93), Float or Complex: y = alpha x +
    (1 - alpha) y_prev as an f64 scan; ValueError ("alpha out of range") unless 0 <= alpha <= 1."""
    dt = np.dtype(dtype)
    return Block(lib().rr_single_pole_iir_create(float(alpha), dt.itemsize), dt, dt)


class BurstDetector(Block):
    """ComplexToMag2 -> SinglePoleIirFilter(alpha) -> the comparison of BurstTagger(threshold) fused into one block
    (rr_burst_detector_create; the burst path of examples/burst_saver.rs:111-123): Complex in, the filtered power out;
    edges() gives the threshold crossings of the most recent work call."""

    def __init__(self, alpha: float, threshold: float):
        super().__init__(lib().rr_burst_detector_create(float(alpha), float(threshold)), np.complex64, np.float32)

    def edges(self):
        """-> (pos: uint64[], val: bool[]) of the most recent work call, ascending, window-relative (rr_burst_edges)"""
        pos, val = _fetch(lib().rr_burst_edges, self._h, np.uint64, np.uint8)
        return pos, val.astype(bool)


BITS_INVERT, BITS_NRZI, BITS_DESCRAMBLE = 1, 2, 4      # RR_BITS_*


def pack_code(code_bits) -> tuple:
    """a sequence of 0/1 -> (packed, length) as the C ABI takes an access code: bit k of the word is code[k], code[0] the
    oldest bit.  Longer than 64 bits: the length is passed on and the library says so."""
    bits = [int(b) for b in code_bits]
    if any(b not in (0, 1) for b in bits):
        raise ValueError("access code bits must be 0 or 1")
    return sum(b << k for k, b in enumerate(bits[:64])), len(bits)


class _TagBlock(Block):
    """a block with a correlator stage: tags() gives the sync-word tags of the most recent work call"""

    def tags(self):
        """-> (pos: uint64[], diffs: uint8[]) of the most recent work call, ascending, window-relative (rr_bit_tags)"""
        return tuple(_fetch(lib().rr_bit_tags, self._h, np.uint64, np.uint8))


def BinarySlicer() -> Block:
    """BinarySlicer::new(src) (src/binary_slicer.rs:8-20): f32 in, u8 out = x > 0.0."""
    return Block(lib().rr_binary_slicer_create(), np.float32, np.uint8)


def NrziDecode() -> Block:
    """NrziDecode::new(src) (src/nrzi.rs:25-42): u8 in, out[n] = 1 ^ in[n] ^ in[n-1]."""
    return Block(lib().rr_nrzi_decode_create(), np.uint8, np.uint8)


class Descrambler(Block):
    """Descrambler::new(src, mask, seed, len) (src/descrambler.rs:50-93): u8 in, u8 out, the self-synchronising LFSR."""

    def __init__(self, mask: int, seed: int, length: int):
        super().__init__(lib().rr_descrambler_create(int(mask), int(seed), int(length)), np.uint8, np.uint8)

    @classmethod
    def g3ruh(cls):
        """Descrambler::g3ruh (src/descrambler.rs:78-88): mask 0x21, seed 0, length 16"""
        return cls(0x21, 0, 16)


class CorrelateAccessCodeTag(_TagBlock):
    """CorrelateAccessCodeTag::new(src, code, tag, allowed_diffs) (src/correlate_access_code.rs:58-119): u8 in, the same u8
    out; tags() gives where the last len(code) bits matched."""

    def __init__(self, code_bits, allowed_diffs: int = 0):
        code, n = pack_code(code_bits)
        super().__init__(lib().rr_correlate_access_code_tag_create(code, n, int(allowed_diffs)), np.uint8, np.uint8)


class BitDecoder(_TagBlock):
    """BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler] -> [CorrelateAccessCodeTag] fused into one block and
    one kernel launch per call (rr_bit_decoder_create; examples/ax25-9600-rx.rs:195-204, examples/il2p-1200-rx.rs:118-126):
    f32 soft symbols in, u8 bits out.  descrambler: (mask, seed, length) or None; code: a sequence of 0/1 or None."""

    def __init__(self, invert: bool = False, nrzi: bool = False, descrambler=None, code=None, allowed_diffs: int = 0):
        flags = (BITS_INVERT if invert else 0) | (BITS_NRZI if nrzi else 0) | (BITS_DESCRAMBLE if descrambler is not None else 0)
        mask, seed, length = descrambler if descrambler is not None else (0, 0, 0)
        packed, n = pack_code(code) if code is not None else (0, 0)
        super().__init__(lib().rr_bit_decoder_create(flags, int(mask), int(seed), int(length), packed, n, int(allowed_diffs)),
                         np.float32, np.uint8)


def NrziEncode() -> Block:
    """NrziEncode::new(src) (src/nrzi.rs:52-69): u8 in, out[n] = out[n-1] ^ (in[n] == 0), out[-1] = 0."""
    return Block(lib().rr_nrzi_encode_create(), np.uint8, np.uint8)


class Scrambler(Block):
    """Scrambler (src/descrambler.rs:95-123): u8 in, u8 out; only the G3RUH form exists in the reference."""

    def __init__(self):
        super().__init__(lib().rr_scrambler_g3ruh_create(), np.uint8, np.uint8)

    @classmethod
    def g3ruh(cls):
        """Scrambler::g3ruh (src/descrambler.rs:106-118): s[n] = in[n] ^ s[n-12] ^ s[n-17], out[n] = s[n-17]"""
        return cls()


FRAME_FCS, FRAME_G3RUH, FRAME_NRZI, FRAME_SYMBOLS = 1, 2, 4, 8      # RR_FRAME_*
# rr_frame_record
FRAME_RECORD = np.dtype([("start", np.uint64), ("len", np.uint64), ("stuffed", np.uint32), ("fcs", np.uint16)], align=True)


class HdlcFramer(Block):
    """FcsAdder -> HdlcFramer -> PduToStream<u8> -> [Scrambler::g3ruh] -> [NrziEncode] -> [Map(bit ? hi : lo)] behind one handle
    (rr_hdlc_framer_create; src/hdlc_framer.rs, examples/g3ruh.rs:250-267; not a stream block: work() raises): a batch of
    packets in, their line bits (u8) or levels (f32, with FRAME_SYMBOLS) out, back to back.  See include/rustradio_amd.h."""

    def __init__(self, flags: int = 0, lo: float = -1.0, hi: float = 1.0):
        super().__init__(lib().rr_hdlc_framer_create(int(flags), float(lo), float(hi)), np.uint8,
                         np.float32 if int(flags) & FRAME_SYMBOLS else np.uint8)
        self.flags = int(flags)

    @property
    def tile_bits(self) -> int:
        """rr_hdlc_framer_dims"""
        t = C.c_size_t(0)
        if lib().rr_hdlc_framer_dims(self._h, C.byref(t)) != 0:
            raise RuntimeError(last_error())
        return t.value

    @staticmethod
    def _desc(starts, lens):
        st = np.ascontiguousarray(starts, np.uintp)
        ln = np.ascontiguousarray(lens, np.uintp)
        if st.ndim != 1 or st.shape != ln.shape:
            raise ValueError("starts and lens must be two sequences of one length")
        return st, ln

    def bound(self, lens) -> int:
        """rr_hdlc_framer_bound: the elements a push of packets of these lengths produces at most"""
        ln = np.ascontiguousarray(lens, np.uintp)
        return lib().rr_hdlc_framer_bound(self._h, _ptr(ln) if len(ln) else None, len(ln))

    def push_dev(self, d_bytes: int, n_bytes: int, starts, lens, d_out: int, out_cap: int, stream: int = 0) -> None:
        """rr_hdlc_framer_push_dev: packet p is d_bytes[starts[p] : starts[p] + lens[p]] (raw device pointers); asynchronous on
        `stream`; records() waits"""
        st, ln = self._desc(starts, lens)
        if lib().rr_hdlc_framer_push_dev(self._h, C.c_void_p(d_bytes), n_bytes, _ptr(st) if len(st) else None,
                                         _ptr(ln) if len(ln) else None, len(st), C.c_void_p(d_out), out_cap, C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def push_buffer(self, data, starts, lens) -> np.ndarray:
        """rr_hdlc_framer_push on a host byte buffer -> the elements the push produced"""
        x = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).ravel()
        st, ln = self._desc(starts, lens)
        cap = self.bound(ln)
        out = np.zeros(max(cap, 1), self.out_dtype)
        produced = C.c_size_t(0)
        if lib().rr_hdlc_framer_push(self._h, _ptr(x) if len(x) else None, len(x), _ptr(st) if len(st) else None,
                                     _ptr(ln) if len(ln) else None, len(st), _ptr(out), cap, C.byref(produced)) != 0:
            raise RuntimeError(last_error())
        return out[:produced.value]

    def push(self, packets) -> np.ndarray:
        """what the chain does to each popped Vec<u8>, for a list of packets in one call -> their frames back to back"""
        pk = [bytes(p) for p in packets]
        lens = np.array([len(p) for p in pk], np.uintp)
        starts = (np.cumsum(lens) - lens).astype(np.uintp)
        return self.push_buffer(b"".join(pk), starts, lens)

    def records(self):
        """-> (FRAME_RECORD per packet of the most recent push, the elements it produced) (rr_hdlc_framer_records; waits)"""
        produced = C.c_size_t(0)
        rec, = _fetch(lib().rr_hdlc_framer_records, self._h, FRAME_RECORD, tail=(C.byref(produced),))
        return rec, produced.value

    def push_kiss(self, kiss_decode: "KissDecode", d_out: int, out_cap: int, stream: int = 0) -> None:
        """rr_hdlc_framer_push_kiss: the packets of the most recent push of a KissDecode, read from its device arena;
        asynchronous on `stream`; records() waits"""
        if lib().rr_hdlc_framer_push_kiss(self._h, kiss_decode._h, C.c_void_p(d_out), out_cap, C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def produced_dev(self) -> int:
        """-> raw device pointer to the elements the most recent push produced, one unsigned long long
        (rr_hdlc_framer_produced_dev): the d_counts of FskTxMulti.push_dev; valid until the next push"""
        return lib().rr_hdlc_framer_produced_dev(self._h)


HDLC_KEEP_CHECKSUM, HDLC_FIX_BITS = 1, 2      # RR_HDLC_*
# rr_hdlc_frame
HDLC_FRAME = np.dtype([("pos", np.uint64), ("start", np.uint64), ("len", np.uint32), ("flags", np.uint32)], align=True)


class HdlcDeframer(Block):
    """HdlcDeframer::new(src, min_size, max_size) with set_keep_checksum / set_fix_bits as flags behind one handle
    (rr_hdlc_deframer_create; src/hdlc_deframer.rs:80-232; not a stream block: work() raises): the next bits of a stream in, one
    per u8, the frames whose closing flag ends inside them out.  The machine, the open gap's bits and the counters stay on the
    device between pushes.  See include/rustradio_amd.h."""

    def __init__(self, min_size: int, max_size: int, flags: int = 0):
        super().__init__(lib().rr_hdlc_deframer_create(int(min_size), int(max_size), int(flags)), np.uint8, np.uint8)
        self.min_size, self.max_size, self.flags = int(min_size), int(max_size), int(flags)

    def dims(self):
        """-> (tile_bits, carry_bits) (rr_hdlc_deframer_dims)"""
        t, c = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_hdlc_deframer_dims(self._h, C.byref(t), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value

    def push_dev(self, d_bits: int, n: int, stream: int = 0) -> None:
        """rr_hdlc_deframer_push_dev: the next n bits from a raw device pointer; asynchronous on `stream`; frames() waits"""
        if lib().rr_hdlc_deframer_push_dev(self._h, C.c_void_p(d_bits), int(n), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, bits):
        """rr_hdlc_deframer_push on host bits -> [(pos, bytes, fixed)] of the frames that ended inside them"""
        x = np.ascontiguousarray(bits, np.uint8).ravel()
        if lib().rr_hdlc_deframer_push(self._h, _ptr(x) if len(x) else None, len(x)) != 0:
            raise ValueError(last_error())
        return self.result()

    def frames(self) -> np.ndarray:
        """-> HDLC_FRAME per frame of the most recent push, ascending by pos (rr_hdlc_frames; waits)"""
        return _fetch(lib().rr_hdlc_frames, self._h, HDLC_FRAME)[0]

    def frame_bytes(self) -> np.ndarray:
        """-> the byte arena of the most recent push, which frames()["start"] indexes (rr_hdlc_frame_bytes; waits)"""
        return _fetch(lib().rr_hdlc_frame_bytes, self._h, np.uint8)[0]

    def bytes_dev(self):
        """-> (raw device pointer or None, bytes) of the same arena (rr_hdlc_bytes_dev); valid until the next push"""
        n = C.c_size_t(0)
        p = lib().rr_hdlc_bytes_dev(self._h, C.byref(n))
        return p, n.value

    def result(self):
        """frames() and frame_bytes() of the most recent push as [(pos, bytes, fixed)]"""
        rec = self.frames()
        arena = self.frame_bytes() if len(rec) else np.zeros(0, np.uint8)
        return [(int(r["pos"]), arena[int(r["start"]):int(r["start"]) + int(r["len"])].tobytes(), bool(r["flags"] & 1)) for r in rec]

    def stats(self):
        """-> (decoded, crc_error, bitfixed) of the handle so far (rr_hdlc_stats; waits)"""
        d, e, f = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        if lib().rr_hdlc_stats(self._h, C.byref(d), C.byref(e), C.byref(f)) != 0:
            raise RuntimeError(last_error())
        return d.value, e.value, f.value


KISS_MAX_LEN = 10000                             # MAX_LEN of src/kiss.rs:6
# rr_kiss_packet
KISS_PACKET = np.dtype([("pos", np.uint64), ("start", np.uint64), ("len", np.uint32), ("in_bytes", np.uint32), ("port", np.uint32),
                        ("reserved", np.uint32)], align=True)
# rr_kiss_frame_record
KISS_FRAME_RECORD = np.dtype([("start", np.uintp), ("len", np.uintp), ("escaped", np.uint32), ("port", np.uint32)], align=True)


class KissDecode(Block):
    """KissFrame -> KissDecode behind one handle (rr_kiss_decode_create; src/kiss.rs:96-228; not a stream block: work() raises):
    the next bytes of a KISS stream in, the packets whose closing FEND lies inside them out.  Whether a FEND has been seen, the
    open gap's bytes and the counters stay on the device between pushes.  See include/rustradio_amd.h."""

    def __init__(self, max_len: int = KISS_MAX_LEN):
        super().__init__(lib().rr_kiss_decode_create(int(max_len)), np.uint8, np.uint8)
        self.max_len = int(max_len)

    def dims(self):
        """-> (tile_bytes, carry_bytes, launches of a push) (rr_kiss_decode_dims)"""
        t, c, k = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        if lib().rr_kiss_decode_dims(self._h, C.byref(t), C.byref(c), C.byref(k)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value, k.value

    def push_dev(self, d_bytes: int, n: int, stream: int = 0) -> None:
        """rr_kiss_decode_push_dev: the next n bytes from a raw device pointer; asynchronous on `stream`; packets() waits"""
        if lib().rr_kiss_decode_push_dev(self._h, C.c_void_p(d_bytes), int(n), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, data):
        """rr_kiss_decode_push on host bytes -> [(pos, port, in_bytes, bytes)] of the packets that ended inside them"""
        x = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).ravel()
        if lib().rr_kiss_decode_push(self._h, _ptr(x) if len(x) else None, len(x)) != 0:
            raise ValueError(last_error())
        return self.result()

    def packets(self) -> np.ndarray:
        """-> KISS_PACKET per packet of the most recent push, ascending by pos (rr_kiss_packets; waits)"""
        return _fetch(lib().rr_kiss_packets, self._h, KISS_PACKET)[0]

    def packet_bytes(self) -> np.ndarray:
        """-> the byte arena of the most recent push, packed in stream order (rr_kiss_packet_bytes; waits)"""
        return _fetch(lib().rr_kiss_packet_bytes, self._h, np.uint8)[0]

    def bytes_dev(self):
        """-> (raw device pointer or None, an upper bound of its bytes) of the same arena (rr_kiss_packet_bytes_dev)"""
        n = C.c_size_t(0)
        p = lib().rr_kiss_packet_bytes_dev(self._h, C.byref(n))
        return p, n.value

    def result(self):
        """packets() and packet_bytes() of the most recent push as [(pos, port, in_bytes, bytes)]"""
        rec = self.packets()
        arena = self.packet_bytes() if len(rec) else np.zeros(0, np.uint8)
        return [(int(r["pos"]), int(r["port"]), int(r["in_bytes"]), arena[int(r["start"]):int(r["start"]) + int(r["len"])].tobytes())
                for r in rec]

    def stats(self):
        """-> (frames, delivered, nondata, bad_escape, overlong) of the handle so far (rr_kiss_decode_stats; waits)"""
        five = (C.c_ulonglong * 5)()
        if lib().rr_kiss_decode_stats(self._h, five) != 0:
            raise RuntimeError(last_error())
        return tuple(int(v) for v in five)


class KissEncode(Block):
    """KissEncode -> PduToStream<u8> behind one handle (rr_kiss_encode_create; src/kiss.rs:247-286; not a stream block: work()
    raises): a batch of packets in, their KISS frames out, back to back.  See include/rustradio_amd.h."""

    def __init__(self):
        super().__init__(lib().rr_kiss_encode_create(), np.uint8, np.uint8)

    def dims(self):
        """-> (tile_bytes, launches of a push) (rr_kiss_encode_dims)"""
        t, k = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_kiss_encode_dims(self._h, C.byref(t), C.byref(k)) != 0:
            raise RuntimeError(last_error())
        return t.value, k.value

    @staticmethod
    def bound(lens) -> int:
        """rr_kiss_encode_bound: the bytes a push of packets of these lengths produces at most"""
        ln = np.ascontiguousarray(lens, np.uintp)
        return lib().rr_kiss_encode_bound(_ptr(ln) if len(ln) else None, len(ln))

    @staticmethod
    def _ports(ports, n):
        if ports is None:
            return None
        po = np.ascontiguousarray(ports, np.uint32)
        if po.shape != (n,):
            raise ValueError("ports must be one per packet")
        return po

    def push_dev(self, d_bytes: int, n_bytes: int, starts, lens, ports, d_out: int, out_cap: int, stream: int = 0) -> None:
        """rr_kiss_encode_push_dev: packet p is d_bytes[starts[p] : starts[p] + lens[p]] (raw device pointers); asynchronous on
        `stream`; records() waits"""
        st, ln = HdlcFramer._desc(starts, lens)
        po = self._ports(ports, len(st))
        if lib().rr_kiss_encode_push_dev(self._h, C.c_void_p(d_bytes), n_bytes, _ptr(st) if len(st) else None,
                                         _ptr(ln) if len(ln) else None, _ptr(po) if po is not None and len(po) else None, len(st),
                                         C.c_void_p(d_out), out_cap, C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push_buffer(self, data, starts, lens, ports=None) -> np.ndarray:
        """rr_kiss_encode_push on a host byte buffer -> the bytes the push produced"""
        x = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).ravel()
        st, ln = HdlcFramer._desc(starts, lens)
        po = self._ports(ports, len(st))
        cap = self.bound(ln)
        out = np.zeros(max(cap, 1), np.uint8)
        produced = C.c_size_t(0)
        if lib().rr_kiss_encode_push(self._h, _ptr(x) if len(x) else None, len(x), _ptr(st) if len(st) else None,
                                     _ptr(ln) if len(ln) else None, _ptr(po) if po is not None and len(po) else None, len(st),
                                     _ptr(out), cap, C.byref(produced)) != 0:
            raise ValueError(last_error())
        return out[:produced.value]

    def push(self, packets, ports=None) -> bytes:
        """what the block does to each popped Vec<u8>, for a list of packets in one call -> their frames back to back"""
        pk = [bytes(p) for p in packets]
        lens = np.array([len(p) for p in pk], np.uintp)
        starts = (np.cumsum(lens) - lens).astype(np.uintp)
        return self.push_buffer(b"".join(pk), starts, lens, ports).tobytes()

    def records(self):
        """-> (KISS_FRAME_RECORD per packet of the most recent push, the bytes it produced) (rr_kiss_encode_records; waits)"""
        produced = C.c_size_t(0)
        rec, = _fetch(lib().rr_kiss_encode_records, self._h, KISS_FRAME_RECORD, tail=(C.byref(produced),))
        return rec, produced.value

    def encode_frames(self, source, d_out: int, out_cap: int, port_of_stream=None, stream: int = 0) -> None:
        """rr_kiss_encode_frames: the frames of the most recent push of an HdlcDeframer or an HdlcReceiver, read from its device
        arena; asynchronous on `stream`; records() waits"""
        po = None if port_of_stream is None else np.ascontiguousarray(port_of_stream, np.uint32)
        if lib().rr_kiss_encode_frames(self._h, source._h, _ptr(po) if po is not None and len(po) else None,
                                       0 if po is None else len(po), C.c_void_p(d_out), out_cap, C.c_void_p(stream)) != 0:
            raise ValueError(last_error())


PWM_SHORT_IS_ZERO, PWM_GAP_DELIMITER = 1, 2      # RR_PWM_*
# rr_pwm_frame
PWM_FRAME = np.dtype([("first_sample", np.uint64), ("start", np.uint64), ("len", np.uint32), ("repeats", np.uint32)], align=True)


class PwmDecoder(Block):
    """PwmDecoder::builder(high_threshold, short_width, long_width, frame_gap, reset_gap) with every builder setting behind one
    handle (rr_pwm_decoder_create; src/pwm_decoder.rs:165-266, 385-513; not a stream block: work() raises): the next samples
    of an OOK power stream in (dtype float32), or of the Complex stream in front of ComplexToMag2 (dtype complex64: the whole
    graph of examples/restaurant_pager.rs), the frames of every transmission whose reset sample lies inside them out.  The
    builder's defaults are supplied here: low_threshold = high_threshold / 2 in f32 and pulse_tolerance = |long - short| / 2
    (:85-88); frame_bits None is gap-delimited.  The slicer, the open frame and the candidate table stay on the device between
    pushes.  See include/rustradio_amd.h."""

    def __init__(self, high_threshold: float, short_width: int, long_width: int, frame_gap: int, reset_gap: int, *,
                 low_threshold=None, pulse_tolerance=None, frame_bits=None, max_frame_bits: int = 4096,
                 max_distinct_frames: int = 256, min_repeats: int = 1, short_is_one: bool = True, delimiter: bool = False,
                 dtype=np.float32):
        dt = np.dtype(dtype)
        high = np.float32(high_threshold)
        low = np.float32(high / np.float32(2.0)) if low_threshold is None else np.float32(low_threshold)
        tol = abs(int(long_width) - int(short_width)) // 2 if pulse_tolerance is None else int(pulse_tolerance)
        if frame_bits is not None and int(frame_bits) == 0:      # (0 is None across the C ABI: validate()'s own refusal, :133-137)
            raise ValueError("PwmDecoder fixed frame length must be greater than zero")
        flags = (0 if short_is_one else PWM_SHORT_IS_ZERO) | (PWM_GAP_DELIMITER if delimiter else 0)
        args = [int(short_width), int(long_width), tol, int(frame_gap), int(reset_gap), 0 if frame_bits is None else int(frame_bits),
                int(max_frame_bits), int(max_distinct_frames), int(min_repeats)]
        if any(a < 0 for a in args):
            raise ValueError("PwmDecoder: a width, gap or count below zero")
        super().__init__(lib().rr_pwm_decoder_create(float(high), float(low), *args, flags, dt.itemsize), dt, np.uint8)

    def dims(self) -> int:
        """-> tile_samples (rr_pwm_decoder_dims)"""
        t = C.c_size_t(0)
        if lib().rr_pwm_decoder_dims(self._h, C.byref(t)) != 0:
            raise RuntimeError(last_error())
        return t.value

    def push_dev(self, d_samples: int, n: int, stream: int = 0) -> None:
        """rr_pwm_decoder_push_dev: the next n samples from a raw device pointer; asynchronous on `stream`; frames() waits"""
        if lib().rr_pwm_decoder_push_dev(self._h, C.c_void_p(d_samples), int(n), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, samples):
        """rr_pwm_decoder_push on host samples -> [(bits: uint8[], repeats, first_sample)] of the transmissions that ended inside them"""
        x = np.ascontiguousarray(samples, self.in_dtype).ravel()
        if lib().rr_pwm_decoder_push(self._h, _ptr(x) if len(x) else None, len(x)) != 0:
            raise ValueError(last_error())
        return self.result()

    def flush(self, stream: int = 0):
        """rr_pwm_decoder_flush: EOF -> the open transmission's candidates, as push() returns them; pushes are refused afterwards"""
        if lib().rr_pwm_decoder_flush(self._h, C.c_void_p(stream)) != 0:
            raise ValueError(last_error())
        return self.result()

    def frames(self) -> np.ndarray:
        """-> PWM_FRAME per frame of the most recent push or flush, in delivery order (rr_pwm_frames; waits)"""
        return _fetch(lib().rr_pwm_frames, self._h, PWM_FRAME)[0]

    def frame_bits(self) -> np.ndarray:
        """-> the bit arena of the most recent push or flush, which frames()["start"] indexes (rr_pwm_frame_bits; waits)"""
        return _fetch(lib().rr_pwm_frame_bits, self._h, np.uint8)[0]

    def bits_dev(self):
        """-> (raw device pointer or None, bits) of the same arena (rr_pwm_bits_dev; waits); valid until the next push"""
        n = C.c_size_t(0)
        p = lib().rr_pwm_bits_dev(self._h, C.byref(n))
        return p, n.value

    def result(self):
        """frames() and frame_bits() of the most recent push or flush as [(bits, repeats, first_sample)]"""
        rec = self.frames()
        arena = self.frame_bits() if len(rec) else np.zeros(0, np.uint8)
        return [(arena[int(r["start"]):int(r["start"]) + int(r["len"])].copy(), int(r["repeats"]), int(r["first_sample"])) for r in rec]


# rr_hdlc_stream_frame
HDLC_STREAM_FRAME =np.dtype([("pos", np.uint64), ("start", np.uint64), ("len", np.uint32), ("flags", np.uint32),
                              ("stream", np.uint32), ("reserved", np.uint32)], align=True)


class HdlcReceiver(Block):
    """BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler] -> HdlcDeframer x nstreams behind one handle
    (rr_hdlc_receiver_create; examples/ax25-9600-rx.rs:195-215; not a stream block: work() raises): the ragged symbol windows
    SymbolSync leaves on the device in, with their counts read there, the checked frames of all streams out.  Every stream's
    state stays on the device between pushes.  descrambler: (mask, seed, length) or None.  See include/rustradio_amd.h."""

    def __init__(self, nstreams: int, min_size: int, max_size: int, invert: bool = False, nrzi: bool = False, descrambler=None,
                 flags: int = 0):
        bits = (BITS_INVERT if invert else 0) | (BITS_NRZI if nrzi else 0) | (BITS_DESCRAMBLE if descrambler is not None else 0)
        mask, seed, length = descrambler if descrambler is not None else (0, 0, 0)
        super().__init__(lib().rr_hdlc_receiver_create(int(nstreams), bits, int(mask), int(seed), int(length), int(min_size),
                                                       int(max_size), int(flags)), np.float32, np.uint8)
        self.nstreams, self.min_size, self.max_size, self.flags = int(nstreams), int(min_size), int(max_size), int(flags)

    def dims(self):
        """-> (tile_bits, carry_bits) (rr_hdlc_receiver_dims)"""
        t, c = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_hdlc_receiver_dims(self._h, C.byref(t), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value

    def push_dev(self, d_syms: int, stride: int, n_cap: int, d_counts=None, stream: int = 0) -> None:
        """rr_hdlc_receiver_push_dev: stream c's next min(d_counts[c], n_cap) symbols at d_syms + c * stride (raw device pointers;
        d_counts: unsigned long long[nstreams], SymbolSync.counts_dev(), or None: n_cap each); asynchronous on `stream`;
        frames() waits"""
        if lib().rr_hdlc_receiver_push_dev(self._h, C.c_void_p(d_syms) if d_syms else None, int(stride), int(n_cap),
                                           C.c_void_p(d_counts) if d_counts else None, C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, syms, counts=None):
        """rr_hdlc_receiver_push on a host array of shape (nstreams, n_cap) (or (n_cap,) for one stream), of which stream c
        holds counts[c] symbols (None: n_cap) -> result()"""
        a = np.ascontiguousarray(syms, np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != self.nstreams:
            raise ValueError("HdlcReceiver.push: one row per stream")
        n = a.shape[1]
        k = None
        if counts is not None:
            if len(counts) != self.nstreams:
                raise ValueError("HdlcReceiver.push: one count per stream")
            k = (C.c_size_t * self.nstreams)(*[int(v) for v in counts])
        if lib().rr_hdlc_receiver_push(self._h, _ptr(a) if n else None, n, n, k) != 0:
            raise ValueError(last_error())
        return self.result()

    def frames(self) -> np.ndarray:
        """-> HDLC_STREAM_FRAME per frame of the most recent push, ascending by (stream, pos) (rr_hdlc_receiver_frames; waits)"""
        return _fetch(lib().rr_hdlc_receiver_frames, self._h, HDLC_STREAM_FRAME)[0]

    def frame_bytes(self) -> np.ndarray:
        """-> the byte arena of the most recent push, which frames()["start"] indexes (rr_hdlc_receiver_frame_bytes; waits)"""
        return _fetch(lib().rr_hdlc_receiver_frame_bytes, self._h, np.uint8)[0]

    def bytes_dev(self):
        """-> (raw device pointer or None, bytes) of the same arena (rr_hdlc_receiver_bytes_dev); valid until the next push"""
        n = C.c_size_t(0)
        p = lib().rr_hdlc_receiver_bytes_dev(self._h, C.byref(n))
        return p, n.value

    def result(self):
        """frames() and frame_bytes() of the most recent push -> per stream [(pos, bytes, fixed)], as HdlcDeframer.result()"""
        rec = self.frames()
        arena = self.frame_bytes() if len(rec) else np.zeros(0, np.uint8)
        out = [[] for _ in range(self.nstreams)]
        for r in rec:
            out[int(r["stream"])].append((int(r["pos"]), arena[int(r["start"]):int(r["start"]) + int(r["len"])].tobytes(),
                                          bool(r["flags"] & 1)))
        return out

    def stats(self) -> np.ndarray:
        """-> uint64[nstreams, 3]: decoded, crc_error, bitfixed of every stream so far (rr_hdlc_receiver_stats; waits)"""
        d, e, f = _fetch(lib().rr_hdlc_receiver_stats, self._h, np.uint64, np.uint64, np.uint64)
        return np.stack([d, e, f], axis=1)

    def consumed(self) -> np.ndarray:
        """-> uint64[nstreams]: symbols every stream has taken so far (rr_hdlc_receiver_consumed; waits)"""
        return _fetch(lib().rr_hdlc_receiver_consumed, self._h, np.uint64)[0]


# rr_il2p_header
IL2P_HEADER = np.dtype({"names": ["pos", "stream", "payload_size", "pid", "control", "flags", "diffs", "dst_ssid", "src_ssid", "raw",
                                  "dst", "src", "reserved"],
                        "formats": [np.uint64, np.uint32, np.uint16, np.uint8, np.uint8, np.uint8, np.uint8, np.uint8, np.uint8,
                                    (np.uint8, 15), "S7", "S7", (np.uint8, 15)],
                        "offsets": [0, 8, 12, 14, 15, 16, 17, 18, 19, 20, 35, 42, 49], "itemsize": 64})


class Il2pReceiver(Block):
    """BinarySlicer -> [XorConst(1)] -> CorrelateAccessCodeTag(il2p SYNC_WORD, "sync", allowed_diffs) -> Il2pDeframer x nstreams
    behind one handle (rr_il2p_receiver_create; examples/il2p-1200-rx.rs:118-137; not a stream block: work() raises): the ragged
    symbol windows SymbolSync leaves on the device in, with their counts read there, the parsed IL2P headers of all streams out.
    Every stream's state stays on the device between pushes.  See include/rustradio_amd.h."""

    def __init__(self, nstreams: int, invert: bool = False, allowed_diffs: int = 0, bit_flags=None):
        bits = (BITS_INVERT if invert else 0) if bit_flags is None else int(bit_flags)
        super().__init__(lib().rr_il2p_receiver_create(int(nstreams), bits, int(allowed_diffs)), np.float32, np.uint8)
        self.nstreams, self.allowed_diffs = int(nstreams), int(allowed_diffs)

    def dims(self):
        """-> (tile_bits, carry_bits) (rr_il2p_receiver_dims)"""
        t, c = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_il2p_receiver_dims(self._h, C.byref(t), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value

    def push_dev(self, d_syms: int, stride: int, n_cap: int, d_counts=None, stream: int = 0) -> None:
        """rr_il2p_receiver_push_dev: stream c's next min(d_counts[c], n_cap) symbols at d_syms + c * stride (raw device pointers;
        d_counts: unsigned long long[nstreams], SymbolSync.counts_dev(), or None: n_cap each); asynchronous on `stream`;
        headers() waits"""
        if lib().rr_il2p_receiver_push_dev(self._h, C.c_void_p(d_syms) if d_syms else None, int(stride), int(n_cap),
                                           C.c_void_p(d_counts) if d_counts else None, C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, syms, counts=None):
        """rr_il2p_receiver_push on a host array of shape (nstreams, n_cap) (or (n_cap,) for one stream), of which stream c
        holds counts[c] symbols (None: n_cap) -> headers()"""
        a = np.ascontiguousarray(syms, np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != self.nstreams:
            raise ValueError("Il2pReceiver.push: one row per stream")
        n = a.shape[1]
        k = None
        if counts is not None:
            if len(counts) != self.nstreams:
                raise ValueError("Il2pReceiver.push: one count per stream")
            k = (C.c_size_t * self.nstreams)(*[int(v) for v in counts])
        if lib().rr_il2p_receiver_push(self._h, _ptr(a) if n else None, n, n, k) != 0:
            raise ValueError(last_error())
        return self.headers()

    def headers(self) -> np.ndarray:
        """-> IL2P_HEADER per header whose 120th bit lay in the most recent push, ascending by (stream, pos)
        (rr_il2p_receiver_headers; waits)"""
        return _fetch(lib().rr_il2p_receiver_headers, self._h, IL2P_HEADER)[0]

    def stats(self) -> np.ndarray:
        """-> uint64[nstreams, 2]: headers delivered, sync tags seen of every stream so far (rr_il2p_receiver_stats; waits)"""
        h, s = _fetch(lib().rr_il2p_receiver_stats, self._h, np.uint64, np.uint64)
        return np.stack([h, s], axis=1)

    def consumed(self) -> np.ndarray:
        """-> uint64[nstreams]: symbols every stream has taken so far (rr_il2p_receiver_consumed; waits)"""
        return _fetch(lib().rr_il2p_receiver_consumed, self._h, np.uint64)[0]


class SymbolSync(Block):
    """SymbolSync::new(src, sps, max_deviation, TedZeroCrossing, IirFilter::new(taps)) x nstreams behind one handle
    (rr_symbol_sync_create; src/symbol_sync.rs:46-217; not a stream block: work() raises): the next n samples of each stream in,
    its symbols (and the clock value that goes with each) out, bit-identical to the reference block's.  Every stream's state stays
    on the device between pushes.  See include/rustradio_amd.h."""

    def __init__(self, sps: float, max_deviation: float, taps, nstreams: int = 1):
        t = np.ascontiguousarray(taps, np.float32).ravel()
        super().__init__(lib().rr_symbol_sync_create(float(sps), float(max_deviation), _ptr(t) if len(t) else None, len(t), int(nstreams)),
                         np.float32, np.float32)
        self.nstreams, self.ntaps = int(nstreams), len(t)

    @property
    def streams_per_wave(self) -> int:
        """rr_symbol_sync_dims: 1 or 64"""
        v = C.c_size_t(0)
        if lib().rr_symbol_sync_dims(self._h, C.byref(v)) != 0:
            raise RuntimeError(last_error())
        return v.value

    def push_dev(self, d_in: int, in_stride: int, n: int, d_syms: int, d_clock, out_stride: int, stream: int = 0) -> None:
        """rr_symbol_sync_push_dev: stream c's next n samples at d_in + c * in_stride (raw device pointers, f32 elements), its
        symbols to d_syms + c * out_stride, its clock values to d_clock + c * out_stride (None: not wanted); asynchronous on
        `stream`; produced() waits"""
        if lib().rr_symbol_sync_push_dev(self._h, C.c_void_p(d_in), int(in_stride), int(n), C.c_void_p(d_syms),
                                         C.c_void_p(d_clock) if d_clock else None, int(out_stride), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, x, clock: bool = True):
        """rr_symbol_sync_push on a host array of shape (nstreams, n) (or (n,) for one stream) -> ([symbols of stream c],
        [clock values of stream c] or None)"""
        a = np.ascontiguousarray(x, np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != self.nstreams:
            raise ValueError("SymbolSync.push: one row per stream")
        n = a.shape[1]
        syms = np.zeros((self.nstreams, max(n, 1)), np.float32)
        clk = np.zeros_like(syms) if clock else None
        produced = (C.c_size_t * self.nstreams)()
        if lib().rr_symbol_sync_push(self._h, _ptr(a) if n else None, n, n, _ptr(syms) if n else None, _ptr(clk) if clock and n else None,
                                     n, produced) != 0:
            raise ValueError(last_error())
        return ([syms[c, :produced[c]].copy() for c in range(self.nstreams)],
                [clk[c, :produced[c]].copy() for c in range(self.nstreams)] if clock else None)

    def produced(self) -> np.ndarray:
        """-> symbols of each stream in the most recent push, uint64[nstreams] (rr_symbol_sync_produced; waits)"""
        out = (C.c_size_t * self.nstreams)()
        total = C.c_size_t(0)
        if lib().rr_symbol_sync_produced(self._h, out, self.nstreams, C.byref(total)) != 0:
            raise RuntimeError(last_error())
        return np.array(out[:total.value], np.uint64)

    def counts_dev(self) -> int:
        """-> raw device pointer to the same counts, unsigned long long[nstreams] (rr_symbol_sync_counts_dev); valid until the
        next push"""
        return lib().rr_symbol_sync_counts_dev(self._h)

    def state(self, stream: int = 0) -> dict:
        """-> the carried state of one stream after the most recent push (rr_debug_symbol_sync_state; waits): clock, stream_pos,
        last_sym_boundary_pos, next_sym_middle (float32), last_sign (bool), hist (float32[ntaps - 1], oldest first)"""
        four = np.zeros(4, np.float32)
        hist = np.zeros(8, np.float32)
        sign, nh = C.c_int(0), C.c_size_t(0)
        if lib().rr_debug_symbol_sync_state(self._h, int(stream), _ptr(four), C.byref(sign), _ptr(hist), len(hist), C.byref(nh)) != 0:
            raise ValueError(last_error())
        return {"clock": four[0], "stream_pos": four[1], "last_sym_boundary_pos": four[2], "next_sym_middle": four[3],
                "last_sign": bool(sign.value), "hist": hist[:nh.value].copy()}


class AfskDemod(Block):
    """Hilbert(hilbert_ntaps, window) -> QuadratureDemod(gain) -> FftFilterFloat(taps) -> AddConst(offset) x nstreams behind one
    handle (rr_afsk_demod_create; examples/ax25-1200-rx.rs:238-247; not a stream block: work() raises): the next n samples of
    each stream in, the soft samples they complete out — n of each, n - 1 for the push that starts the streams.  The bits do not
    depend on how a stream is cut into pushes.  Every stream's latest samples stay on the device.  See include/rustradio_amd.h."""

    def __init__(self, nstreams: int, hilbert_ntaps: int, taps, gain: float = 1.0, offset: float = 0.0,
                 window: int = WIN_HAMMING, window_parm: float = 0.0):
        t = np.ascontiguousarray(taps, np.float32).ravel()
        super().__init__(lib().rr_afsk_demod_create(int(nstreams), int(hilbert_ntaps), int(window), float(window_parm), float(gain),
                                                    _ptr(t) if len(t) else None, len(t), float(offset)), np.float32, np.float32)
        self.nstreams, self.ntaps, self.hilbert_ntaps = int(nstreams), len(t), int(hilbert_ntaps)

    def dims(self):
        """-> (tile_samples, carry_samples) (rr_afsk_demod_dims)"""
        t, c = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_afsk_demod_dims(self._h, C.byref(t), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value

    def push_dev(self, d_in: int, in_stride: int, n: int, d_out: int, out_stride: int, stream: int = 0) -> int:
        """rr_afsk_demod_push_dev: stream c's next n samples at d_in + c * in_stride (raw device pointers, f32 elements), its
        outputs to d_out + c * out_stride; asynchronous on `stream` -> produced, the n of the following SymbolSync.push_dev"""
        k = C.c_size_t(0)
        if lib().rr_afsk_demod_push_dev(self._h, C.c_void_p(d_in), int(in_stride), int(n), C.c_void_p(d_out), int(out_stride),
                                        C.byref(k), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())
        return k.value

    def push(self, x) -> np.ndarray:
        """rr_afsk_demod_push on a host array of shape (nstreams, n) (or (n,) for one stream) -> float32 (nstreams, produced)"""
        a = np.ascontiguousarray(x, np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != self.nstreams:
            raise ValueError("AfskDemod.push: one row per stream")
        n = a.shape[1]
        out = np.zeros((self.nstreams, max(n, 1)), np.float32)
        k = C.c_size_t(0)
        if lib().rr_afsk_demod_push(self._h, _ptr(a) if n else None, n, n, _ptr(out) if n else None, n, C.byref(k)) != 0:
            raise ValueError(last_error())
        return out[:, :k.value].copy()


class AmDemod(Block):
    """norm -> FftFilterFloat(taps) -> RationalResampler(interp, deci) -> MultiplyConst(scale) x nstreams behind one handle
    (rr_am_demod_create; examples/airspy_am_decode.rs; not a stream block: work() raises): the next n Complex samples of each
    stream in, the audio samples they complete out — ceil(N interp / deci) of each after N samples in all.  Only the filter outputs
    the resampler picks are computed.  The bits do not depend on how a stream is cut into pushes.  Every stream's latest
    magnitudes stay on the device.  See include/rustradio_amd.h."""

    def __init__(self, nstreams: int, taps, interp: int = 1, deci: int = 1, scale: float = 1.0):
        t = np.ascontiguousarray(taps, np.float32).ravel()
        super().__init__(lib().rr_am_demod_create(int(nstreams), _ptr(t) if len(t) else None, len(t), int(interp), int(deci),
                                                  float(scale)), np.complex64, np.float32)
        g = math.gcd(int(interp), int(deci))
        self.nstreams, self.ntaps, self.interp, self.deci = int(nstreams), len(t), int(interp) // g, int(deci) // g
        self.total = 0                         # samples every stream has taken

    def dims(self):
        """-> (tile_outputs, carry_samples) (rr_am_demod_dims)"""
        t, c = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_am_demod_dims(self._h, C.byref(t), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return t.value, c.value

    def count(self, n: int) -> int:
        """outputs of each stream a push of n samples would deliver now"""
        up = lambda N: (N * self.interp + self.deci - 1) // self.deci
        return up(self.total + int(n)) - up(self.total)

    def push_dev(self, d_in: int, in_stride: int, n: int, d_out: int, out_stride: int, stream: int = 0) -> int:
        """rr_am_demod_push_dev: stream c's next n samples at d_in + c * in_stride (raw device pointers, Complex elements), its
        outputs to d_out + c * out_stride (f32 elements); asynchronous on `stream` -> produced"""
        k = C.c_size_t(0)
        if lib().rr_am_demod_push_dev(self._h, C.c_void_p(d_in), int(in_stride), int(n), C.c_void_p(d_out), int(out_stride),
                                      C.byref(k), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())
        self.total += int(n)
        return k.value

    def push(self, x) -> np.ndarray:
        """rr_am_demod_push on a host array of shape (nstreams, n) (or (n,) for one stream) -> float32 (nstreams, produced)"""
        a = np.ascontiguousarray(x, np.complex64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[0] != self.nstreams:
            raise ValueError("AmDemod.push: one row per stream")
        n = a.shape[1]
        cap = self.count(n)
        out = np.zeros((self.nstreams, max(cap, 1)), np.float32)
        k = C.c_size_t(0)
        if lib().rr_am_demod_push(self._h, _ptr(a) if n else None, n, n, _ptr(out) if cap else None, cap, C.byref(k)) != 0:
            raise ValueError(last_error())
        self.total += n
        return out[:, :k.value].copy()


FSK_TX_DIRECT, FSK_TX_AFSK = 0, 1      # RR_FSK_TX_*


class FskTx(Block):
    """The modulators of the reference's packet transmitters in PDU form (rr_fsk_tx_create; not a stream block: work() raises):
    u8 line bits in (HdlcFramer's, without FRAME_SYMBOLS; nonzero = 1), Complex baseband out.
      FSK_TX_AFSK    RationalResampler(interp1, deci1) -> Map(bit ? hi : lo) -> Vco(k1) -> .re -> MultiplyConst(gain) ->
                     RationalResampler(interp2, deci2) -> Vco(k2)          (examples/bell202.rs:166-183); the audio is an output too
      FSK_TX_DIRECT  RationalResampler -> Map -> Vco(k1) -> MultiplyConst(gain) -> RationalResampler   (examples/g3ruh.rs:256-272)
    Every push emits everything its bits produce; both phases stay on the device.  See include/rustradio_amd.h."""

    def __init__(self, mode: int, interp1: int, deci1: int, lo: float, hi: float, k1: float, gain: float, interp2: int = 1,
                 deci2: int = 1, k2: float = 0.0):
        super().__init__(lib().rr_fsk_tx_create(int(mode), int(interp1), int(deci1), float(lo), float(hi), _f64_bits(float(k1)),
                                                float(gain), int(interp2), int(deci2), _f64_bits(float(k2))), np.uint8, np.complex64)
        self.mode = int(mode)

    def dims(self):
        """-> (audio_tile, out_tile, scan_chunk_tiles) (rr_fsk_tx_dims)"""
        a, o, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_dims(self._h, C.byref(a), C.byref(o), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return a.value, o.value, c.value

    def count(self, n_bits: int):
        """-> (n_audio, n_out) of the NEXT push of n_bits (rr_fsk_tx_count)"""
        a, o = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_count(self._h, int(n_bits), C.byref(a), C.byref(o)) != 0:
            raise ValueError(last_error())
        return a.value, o.value

    def push_dev(self, d_bits: int, n_bits: int, d_out: int, out_cap: int, d_audio: int = 0, audio_cap: int = 0, stream: int = 0):
        """rr_fsk_tx_push_dev on raw device pointers (d_audio 0: no audio output); asynchronous on `stream` -> (n_out, n_audio)"""
        o, a = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_push_dev(self._h, C.c_void_p(d_bits), int(n_bits), C.c_void_p(d_out), int(out_cap), C.c_void_p(d_audio),
                                    int(audio_cap), C.byref(o), C.byref(a), C.c_void_p(stream)) != 0:
            raise ValueError(last_error())
        return o.value, a.value

    def push(self, bits, audio: bool = False):
        """rr_fsk_tx_push on a host array of u8 bits -> complex64 out, or (out, float32 audio) with audio=True (AFSK mode)"""
        b = np.ascontiguousarray(bits, np.uint8).ravel()
        na, no = self.count(len(b))
        out = np.zeros(max(no, 1), np.complex64)
        aud = np.zeros(max(na, 1), np.float32) if audio else None
        o, a = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_push(self._h, _ptr(b) if len(b) else None, len(b), _ptr(out), no, _ptr(aud) if audio else None,
                                na if audio else 0, C.byref(o), C.byref(a)) != 0:
            raise ValueError(last_error())
        return (out[:o.value].copy(), aud[:a.value].copy()) if audio else out[:o.value].copy()


class FskTxMulti(Block):
    """FskTx x nstreams of one parameter set behind one handle (rr_fsk_tx_multi_create; not a stream block: work() raises): ragged
    pushes of u8 line bits in, each stream's Complex baseband (and, in AFSK mode, its audio) out.  Every stream's state stays on
    the device and the bit counts of a push are read there, so HdlcFramer.push_dev -> FskTxMulti.push_dev needs no host read
    (HdlcFramer.produced_dev).  See include/rustradio_amd.h."""

    def __init__(self, nstreams: int, mode: int, interp1: int, deci1: int, lo: float, hi: float, k1: float, gain: float,
                 interp2: int = 1, deci2: int = 1, k2: float = 0.0):
        super().__init__(lib().rr_fsk_tx_multi_create(int(nstreams), int(mode), int(interp1), int(deci1), float(lo), float(hi),
                                                      _f64_bits(float(k1)), float(gain), int(interp2), int(deci2),
                                                      _f64_bits(float(k2))), np.uint8, np.complex64)
        self.nstreams, self.mode = int(nstreams), int(mode)

    def dims(self):
        """-> (audio_tile, out_tile, scan_chunk_tiles) (rr_fsk_tx_multi_dims)"""
        a, o, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_multi_dims(self._h, C.byref(a), C.byref(o), C.byref(c)) != 0:
            raise RuntimeError(last_error())
        return a.value, o.value, c.value

    def bound(self, n_cap: int):
        """-> (audio_cap, out_cap): the most one stream makes from n_cap bits (rr_fsk_tx_multi_bound)"""
        a, o = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_fsk_tx_multi_bound(self._h, int(n_cap), C.byref(a), C.byref(o)) != 0:
            raise RuntimeError(last_error())
        return a.value, o.value

    def push_dev(self, d_bits: int, bits_stride: int, n_cap: int, d_counts, d_out: int, out_stride: int, d_audio: int = 0,
                 audio_stride: int = 0, stream: int = 0) -> None:
        """rr_fsk_tx_multi_push_dev: stream c's next min(d_counts[c], n_cap) bits at d_bits + c * bits_stride (raw device pointers;
        d_counts: unsigned long long[nstreams], e.g. HdlcFramer.produced_dev(), or None: n_cap each), its outputs to d_out + c *
        out_stride, its audio to d_audio + c * audio_stride (0: not wanted); asynchronous on `stream`; counts() waits"""
        if lib().rr_fsk_tx_multi_push_dev(self._h, C.c_void_p(d_bits) if d_bits else None, int(bits_stride), int(n_cap),
                                          C.c_void_p(d_counts) if d_counts else None, C.c_void_p(d_out) if d_out else None,
                                          int(out_stride), C.c_void_p(d_audio) if d_audio else None, int(audio_stride),
                                          C.c_void_p(stream)) != 0:
            raise ValueError(last_error())

    def push(self, bits, counts=None, audio: bool = False):
        """rr_fsk_tx_multi_push on a host array of shape (nstreams, n_cap) (or (n_cap,) for one stream), of which stream c holds
        counts[c] bits (None: n_cap) -> [complex64 out of stream c], or ([out], [float32 audio]) with audio=True (AFSK mode)"""
        b = np.ascontiguousarray(bits, np.uint8)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        if b.ndim != 2 or b.shape[0] != self.nstreams:
            raise ValueError("FskTxMulti.push: one row per stream")
        n = b.shape[1]
        k = None
        if counts is not None:
            if len(counts) != self.nstreams:
                raise ValueError("FskTxMulti.push: one count per stream")
            k = (C.c_size_t * self.nstreams)(*[int(v) for v in counts])
        ac, oc = self.bound(n)
        out = np.zeros((self.nstreams, max(oc, 1)), np.complex64)
        aud = np.zeros((self.nstreams, max(ac, 1)), np.float32) if audio else None
        no, na = (C.c_size_t * self.nstreams)(), (C.c_size_t * self.nstreams)()
        if lib().rr_fsk_tx_multi_push(self._h, _ptr(b) if n else None, n, n, k, _ptr(out), out.shape[1], _ptr(aud) if audio else None,
                                      aud.shape[1] if audio else 0, no, na) != 0:
            raise ValueError(last_error())
        outs = [out[c, :no[c]].copy() for c in range(self.nstreams)]
        return (outs, [aud[c, :na[c]].copy() for c in range(self.nstreams)]) if audio else outs

    def counts(self) -> np.ndarray:
        """-> uint64[nstreams, 2]: (n_audio, n_out) of each stream in the most recent push (rr_fsk_tx_multi_counts; waits)"""
        a, o = _fetch(lib().rr_fsk_tx_multi_counts, self._h, np.uintp, np.uintp)
        return np.stack([a, o], axis=1).astype(np.uint64)

    def counts_dev(self) -> int:
        """-> raw device pointer to the same counts, unsigned long long[2][nstreams], audio counts then output counts
        (rr_fsk_tx_multi_counts_dev); valid until the next push"""
        return lib().rr_fsk_tx_multi_counts_dev(self._h)

    def positions(self) -> np.ndarray:
        """-> uint64[nstreams, 3]: bits taken, audio samples and outputs made by each stream so far (rr_fsk_tx_multi_positions;
        waits)"""
        b, a, o = _fetch(lib().rr_fsk_tx_multi_positions, self._h, np.uint64, np.uint64, np.uint64)
        return np.stack([b, a, o], axis=1)


WPCR_MAX_LEN = 512_000     # samples of one burst: the reference's stream capacity in f32
# rr_wpcr_result
WPCR_RESULT = np.dtype([("ok", np.int32), ("bin", np.uint32), ("sps", np.float32), ("phase0", np.float32), ("phase", np.float32),
                        ("frequency", np.float32), ("nsyms", np.uint64)], align=True)


class Wpcr(Block):
    """Wpcr::builder(src)[.samp_rate(s)] (src/wpcr.rs:84-239): whole-packet clock recovery over a batch of bursts, the PDU form
    (rr_wpcr_create; not a stream block: work() raises).  The symbols are picked by the drift-free clock p0 + i * sps; see
    include/rustradio_amd.h for where that differs from the reference's f32 accumulator."""

    def __init__(self, samp_rate=None):
        super().__init__(lib().rr_wpcr_create(float("nan") if samp_rate is None else float(samp_rate)), np.float32, np.float32)
        self.samp_rate = samp_rate
        self._lens = None           # of the most recent call (spectrum() sizes its buffer by them)

    def _desc(self, starts, lens, mids):
        st = np.ascontiguousarray(starts, np.uintp)
        ln = np.ascontiguousarray(lens, np.uintp)
        if st.ndim != 1 or st.shape != ln.shape:
            raise ValueError("starts and lens must be two sequences of one length")
        md = None if mids is None else np.ascontiguousarray(mids, np.float32)
        if md is not None and md.shape != st.shape:
            raise ValueError("mids must have one entry per burst")
        return st, ln, md

    def process_dev(self, d_samples: int, n_total: int, starts, lens, mids, d_syms: int, stream: int = 0) -> None:
        """rr_wpcr_process_dev: burst b is d_samples[starts[b] : starts[b] + lens[b]] (raw device pointers to n_total f32 each);
        its symbols go to d_syms[starts[b] :].  Asynchronous on `stream`; results() waits."""
        st, ln, md = self._desc(starts, lens, mids)
        if lib().rr_wpcr_process_dev(self._h, C.c_void_p(d_samples), n_total, _ptr(st), _ptr(ln), None if md is None else _ptr(md),
                                     len(st), C.c_void_p(d_syms), C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())
        self._lens = ln

    def process_buffer(self, samples: np.ndarray, starts, lens, mids=None) -> np.ndarray:
        """rr_wpcr_process on host arrays -> syms, the same geometry as `samples`"""
        x = np.ascontiguousarray(samples, np.float32)
        st, ln, md = self._desc(starts, lens, mids)
        syms = np.zeros(max(len(x), 1), np.float32)
        if lib().rr_wpcr_process(self._h, _ptr(x), len(x), _ptr(st), _ptr(ln), None if md is None else _ptr(md), len(st),
                                 _ptr(syms)) != 0:
            raise RuntimeError(last_error())
        self._lens = ln
        return syms[:len(x)]

    def results(self) -> np.ndarray:
        """one WPCR_RESULT record per burst of the most recent process call (rr_wpcr_results; waits for it)"""
        return _fetch(lib().rr_wpcr_results, self._h, WPCR_RESULT)[0]

    def tags(self, r) -> dict:
        """the tags Wpcr pushes with a packet (wpcr.rs:187-194) from one result record"""
        t = {"sps": r["sps"], "phase": r["phase"]}
        if self.samp_rate is not None:
            t["frequency"] = r["frequency"]
        return t

    def process(self, bursts, mids=None) -> list:
        """what Wpcr::work does to each popped Vec<Float>, for a list of bursts in one call -> per burst (symbols, tags) or
        None (the reference pushes nothing)"""
        arrs = [np.ascontiguousarray(b, np.float32).ravel() for b in bursts]
        lens = np.array([len(a) for a in arrs], np.uintp)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uintp) if len(arrs) else np.zeros(0, np.uintp)
        x = np.concatenate(arrs) if arrs else np.zeros(0, np.float32)
        syms = self.process_buffer(x, starts, lens, mids)
        out = []
        for s, r in zip(starts, self.results()):
            out.append((syms[int(s):int(s) + int(r["nsyms"])].copy(), self.tags(r)) if r["ok"] else None)
        return out

    def process_pdus(self, pdus: "StreamToPdu", d_syms: int, stream: int = 0) -> None:
        """rr_wpcr_process_pdus: Midpointer -> Wpcr over the PDUs of the most recent push of `pdus`, on its arena; d_syms is a raw
        device pointer to as many f32 as the arena holds.  results() then has one record per PDU with ok != 0."""
        if lib().rr_wpcr_process_pdus(self._h, pdus._h, C.c_void_p(d_syms), C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())
        self._lens = None

    def pack(self, d_syms: int, d_out: int, out_cap: int, stream: int = 0):
        """rr_wpcr_pack_dev: PduToStream over the most recent process call -> (produced, pdu_start: uint64[], pdu_len: uint64[]):
        the symbols of every burst with ok and nsyms > 0 back to back in d_out (raw device pointers), and where each begins"""
        produced, npdus = C.c_size_t(0), C.c_size_t(0)
        cap = len(self.results())
        st = np.zeros(max(cap, 1), np.uintp)
        ln = np.zeros(max(cap, 1), np.uintp)
        if lib().rr_wpcr_pack_dev(self._h, C.c_void_p(d_syms), C.c_void_p(d_out), out_cap, C.byref(produced), _ptr(st), _ptr(ln), cap,
                                  C.byref(npdus), C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())
        return produced.value, st[:npdus.value].astype(np.uint64), ln[:npdus.value].astype(np.uint64)

    def spectrum(self, burst: int) -> np.ndarray:
        """rr_debug_wpcr_spectrum: the f32 magnitudes mag[0 : N // 2] the decision for `burst` of the most recent call was taken on"""
        n = C.c_size_t(0)
        known = self._lens is not None and 0 <= burst < len(self._lens)
        mag = np.zeros(max((int(self._lens[burst]) - 1) // 2, 1) if known else 1, np.float32)
        if lib().rr_debug_wpcr_spectrum(self._h, burst, _ptr(mag), len(mag), C.byref(n)) != 0:
            raise RuntimeError(last_error())
        return mag[:n.value]


PDU_MIDPOINT = 1            # RR_PDU_MIDPOINT
PDU_MAX_WINDOW = 1_024_000  # samples of one push: the f32 stream capacity
# rr_pdu_record
PDU_RECORD = np.dtype([("start", np.uint64), ("len", np.uint64), ("stream_pos", np.uint64), ("ok", np.int32), ("mean", np.float32),
                       ("mid", np.float32), ("nlow", np.uint64)], align=True)


class StreamToPdu(Block):
    """BurstTagger(threshold) -> StreamToPdu(max_size, tail) -> [Midpointer] behind one handle (rr_stream_to_pdu_create; not a
    stream block: work() raises): f32 data and an f32 trigger in, one window of both per push; the PDUs a push completes lie in
    one device arena, a burst begun in an earlier push whole.  See include/rustradio_amd.h for the rules."""

    def __init__(self, threshold: float, max_size: int, tail: int, flags: int = 0):
        super().__init__(lib().rr_stream_to_pdu_create(float(threshold), int(max_size), int(tail), int(flags)), np.float32, np.float32)
        self.flags = flags

    def push_dev(self, d_data: int, d_trigger: int, n: int, stream: int = 0) -> None:
        """rr_stream_to_pdu_push_dev: raw device pointers to n f32 each; asynchronous on `stream`; records() waits"""
        if lib().rr_stream_to_pdu_push_dev(self._h, C.c_void_p(d_data), C.c_void_p(d_trigger), n, C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def push(self, data: np.ndarray, trigger: np.ndarray) -> np.ndarray:
        """rr_stream_to_pdu_push on host arrays of one length -> records()"""
        x = np.ascontiguousarray(data, np.float32).ravel()
        t = np.ascontiguousarray(trigger, np.float32).ravel()
        if x.shape != t.shape:
            raise ValueError("data and trigger must have one length")
        if lib().rr_stream_to_pdu_push(self._h, _ptr(x) if len(x) else None, _ptr(t) if len(t) else None, len(x)) != 0:
            raise RuntimeError(last_error())
        return self.records()

    def records(self) -> np.ndarray:
        """one PDU_RECORD per PDU the most recent push completed, ascending (rr_pdu_records; waits for it)"""
        return _fetch(lib().rr_pdu_records, self._h, PDU_RECORD)[0]

    def edges(self):
        """-> (pos: uint64[], val: bool[]) of the most recent push, ascending, window-relative (rr_pdu_edges)"""
        pos, val = _fetch(lib().rr_pdu_edges, self._h, np.uint64, np.uint8)
        return pos, val.astype(bool)

    def arena_dev(self):
        """-> (raw device pointer or None, n_total) of the most recent push's arena (rr_pdu_arena_dev); valid until the next push"""
        n = C.c_size_t(0)
        p = lib().rr_pdu_arena_dev(self._h, C.byref(n))
        return p, n.value

    def pdu(self, i: int, rec=None) -> np.ndarray:
        """the samples of PDU i of the most recent push (rr_pdu_fetch)"""
        r = self.records() if rec is None else rec
        if not 0 <= i < len(r):
            raise IndexError("no such PDU in the most recent push")
        out = np.zeros(max(int(r[i]["len"]), 1), np.float32)
        if lib().rr_pdu_fetch(self._h, i, _ptr(out), int(r[i]["len"])) != 0:
            raise RuntimeError(last_error())
        return out[:int(r[i]["len"])]

    def ranks(self, i: int):
        """rr_debug_pdu_ranks: (low, high), the two elements Midpointer's offset of PDU i of the most recent push was made of"""
        lh = np.zeros(2, np.float32)
        if lib().rr_debug_pdu_ranks(self._h, i, C.c_void_p(lh.ctypes.data), C.c_void_p(lh.ctypes.data + 4)) != 0:
            raise RuntimeError(last_error())
        return lh[0], lh[1]


class StreamToPduC32(StreamToPdu):
    """StreamToPdu<Complex> (rr_stream_to_pdu_c32_create): the f32 trigger, the edges, the records and the carried state of
    StreamToPdu; the data, the arena and the payloads are complex64.  No Midpointer (a block over Vec<Float>)."""

    def __init__(self, threshold: float, max_size: int, tail: int):
        Block.__init__(self, lib().rr_stream_to_pdu_c32_create(float(threshold), int(max_size), int(tail)), np.complex64, np.complex64)
        self.flags = 0

    def push(self, data: np.ndarray, trigger: np.ndarray) -> np.ndarray:
        """rr_stream_to_pdu_push_c32 on host arrays of one length -> records()"""
        x = np.ascontiguousarray(data, np.complex64).ravel()
        t = np.ascontiguousarray(trigger, np.float32).ravel()
        if x.shape != t.shape:
            raise ValueError("data and trigger must have one length")
        if lib().rr_stream_to_pdu_push_c32(self._h, _ptr(x) if len(x) else None, _ptr(t) if len(t) else None, len(x)) != 0:
            raise RuntimeError(last_error())
        return self.records()

    def pdu(self, i: int, rec=None) -> np.ndarray:
        """the samples of PDU i of the most recent push (rr_pdu_fetch_c32)"""
        r = self.records() if rec is None else rec
        if not 0 <= i < len(r):
            raise IndexError("no such PDU in the most recent push")
        out = np.zeros(max(int(r[i]["len"]), 1), np.complex64)
        if lib().rr_pdu_fetch_c32(self._h, i, _ptr(out), int(r[i]["len"])) != 0:
            raise RuntimeError(last_error())
        return out[:int(r[i]["len"])]


TAGS_DROP, TAGS_FORWARD, TAGS_FRAMES, TAGS_SHIFT = 0, 1, 2, 3      # rr_tag_rule


class Delay(Block):
    """Delay::new(src, delay) (rr_delay_create; src/delay.rs): `delay` zero elements, then the input, for a dtype of 1, 4 or 8
    bytes.  ValueError ("unsupported element size", "delay: more than 1,024,000 samples")."""

    def __init__(self, delay: int, dtype=np.complex64):
        dt = np.dtype(dtype)
        super().__init__(lib().rr_delay_create(int(delay), dt.itemsize), dt, dt)
        self.delay = int(delay)

    def tag_rule(self):
        """-> (rule, param) of rr_block_tag_rule: (TAGS_SHIFT, delay)"""
        p = C.c_size_t(0)
        return lib().rr_block_tag_rule(self._h, C.byref(p)), p.value


class BurstSaver(StreamToPduC32):
    """The sample-rate path of examples/burst_saver.rs behind one handle (rr_burst_saver_create): Tee -> [ComplexToMag2 ->
    SinglePoleIirFilter(alpha)] and [Delay(delay)] -> BurstTagger(threshold) -> StreamToPdu<Complex>(max_size, tail).  complex64
    windows in; records(), edges(), arena_dev() and pdu() as StreamToPduC32; save() is PduWriter."""

    def __init__(self, alpha: float, threshold: float, delay: int, max_size: int, tail: int):
        Block.__init__(self, lib().rr_burst_saver_create(float(alpha), float(threshold), int(delay), int(max_size), int(tail)),
                       np.complex64, np.complex64)
        self.flags = 0
        self.delay = int(delay)
        self._written = 0

    def push_dev(self, d_in: int, n: int, d_env: int = 0, stream: int = 0) -> None:
        """rr_burst_saver_push_dev: a raw device pointer to n complex64, and 0 or one to n f32 that receive the envelope;
        asynchronous on `stream`; records() waits"""
        if lib().rr_burst_saver_push_dev(self._h, C.c_void_p(d_in), n, C.c_void_p(d_env), C.c_void_p(stream)) != 0:
            raise RuntimeError(last_error())

    def push(self, x: np.ndarray, env: bool = False):
        """rr_burst_saver_push on a host window -> records(), or (records(), envelope) with env=True"""
        x = np.ascontiguousarray(x, np.complex64).ravel()
        e = np.zeros(max(len(x), 1), np.float32) if env else None
        if lib().rr_burst_saver_push(self._h, _ptr(x) if len(x) else None, len(x), _ptr(e) if env else None) != 0:
            raise RuntimeError(last_error())
        return (self.records(), e[:len(x)]) if env else self.records()

    def dims(self, n: int):
        """-> (tile, kernel launches of a push of n samples) (rr_burst_saver_dims)"""
        t, k = C.c_size_t(0), C.c_size_t(0)
        if lib().rr_burst_saver_dims(self._h, int(n), C.byref(t), C.byref(k)) != 0:
            raise RuntimeError(last_error())
        return t.value, k.value

    def save(self, directory) -> list:
        """PduWriter (src/pdu_writer.rs:41-69) over the PDUs of the most recent push: one file each, named
        <microseconds since the epoch>-<files written so far>, opened create-new, holding the samples as Sample::serialize
        writes them (interleaved little-endian f32 re, im) -> the paths written"""
        import os
        import time
        paths = []
        rec = self.records()
        for i in range(len(rec)):
            name = os.path.join(os.fspath(directory), f"{time.time_ns() // 1000}-{self._written}")
            with open(name, "xb") as f:
                f.write(self.pdu(i, rec).astype("<c8").tobytes())
            self._written += 1
            paths.append(name)
        return paths


def FmChainU8(taps, interp: int, deci: int, gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    """RtlSdrDecode -> FmChain fused (examples/rtl_fm.rs:328-419): RTL-SDR bytes in, f32 out; windows,
    consumed and the WAIT_SRC need count bytes."""
    t = np.ascontiguousarray(taps, np.complex64)
    return Block(lib().rr_fm_chain_u8_create(_ptr(t), len(t), interp, deci, gain, mode), np.uint8, np.float32)


def HilbertFir(hilbert_ntaps: int, taps, deci: int = 1, translate=None, wtype: int = WIN_HAMMING, parm: float = 0.0,
               rotator: int = ROT_REPLAY) -> Block:
    """Hilbert(hilbert_ntaps, wtype) -> FirFilter<Complex>(taps, deci[, translate]) fused into one composite
    decimating FIR on the real input (examples/ax25-1200-rx.rs:238-247 wiring); f32 in, Complex out."""
    t = np.ascontiguousarray(taps, np.complex64)
    fs, f = translate if translate is not None else (0.0, 0.0)
    h = lib().rr_hilbert_fir_create(hilbert_ntaps, wtype, parm, _ptr(t), len(t), deci,
                                    1 if translate is not None else 0, fs, f)
    b = Block(h, np.float32, np.complex64)
    if translate is not None and lib().rr_fir_set_rotator_mode(b._h, rotator) != 0:
        raise ValueError(last_error())
    return b


def FmMulti(taps_per_channel, interp: int, deci: int, gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    """N fused FM chains on one shared input (Tee + N x FmChain); taps_per_channel = [N][ntaps].
    work() returns out with shape (N, produced); work_dev() takes N windows of out_cap elements."""
    t = np.ascontiguousarray(taps_per_channel, np.complex64)
    if t.ndim != 2:
        raise ValueError("taps_per_channel must be [nchan][ntaps]")
    h = lib().rr_fm_multi_create(_ptr(t), t.shape[0], t.shape[1], interp, deci, gain, mode)
    return Block(h, np.complex64, np.float32)


def FmMultiU8(taps_per_channel, interp: int, deci: int, gain: float = 1.0, mode: int = ATAN2_EXACT) -> Block:
    """RtlSdrDecode -> Tee -> N x FmChain fused: RTL-SDR bytes in, N f32 windows out (windows, consumed and the
    WAIT_SRC need count bytes)."""
    t = np.ascontiguousarray(taps_per_channel, np.complex64)
    if t.ndim != 2:
        raise ValueError("taps_per_channel must be [nchan][ntaps]")
    h = lib().rr_fm_multi_u8_create(_ptr(t), t.shape[0], t.shape[1], interp, deci, gain, mode)
    return Block(h, np.uint8, np.float32)


def Channelizer(taps_per_channel, interp: int, deci: int) -> Block:
    """Tee + N x (FftFilter(taps_c) -> RationalResampler(interp, deci)) fused, Complex (baseband) outputs;
    taps_per_channel = [N][ntaps].  work() returns out with shape (N, produced); work_dev() takes N windows of
    out_cap elements.  One channel is the fused FftFilter -> RationalResampler block."""
    t = np.ascontiguousarray(taps_per_channel, np.complex64)
    if t.ndim != 2:
        raise ValueError("taps_per_channel must be [nchan][ntaps]")
    h = lib().rr_channelizer_create(_ptr(t), t.shape[0], t.shape[1], interp, deci)
    return Block(h, np.complex64, np.complex64)


def ChannelizerU8(taps_per_channel, interp: int, deci: int) -> Block:
    """RtlSdrDecode -> Channelizer fused: RTL-SDR bytes in, N Complex windows out (windows, consumed and the
    WAIT_SRC need count bytes)."""
    t = np.ascontiguousarray(taps_per_channel, np.complex64)
    if t.ndim != 2:
        raise ValueError("taps_per_channel must be [nchan][ntaps]")
    h = lib().rr_channelizer_u8_create(_ptr(t), t.shape[0], t.shape[1], interp, deci)
    return Block(h, np.uint8, np.complex64)


def _fm_receiver(create, in_dtype, taps_per_channel, rf_interp, rf_deci, audio_taps, audio_interp, audio_deci, gain, mode, scale):
    t = np.ascontiguousarray(taps_per_channel, np.complex64)
    if t.ndim != 2:
        raise ValueError("taps_per_channel must be [nchan][ntaps]")
    a = np.ascontiguousarray(audio_taps, np.float32)
    if a.ndim != 1:
        raise ValueError("audio_taps must be one set of taps, shared by the channels")
    h = create(_ptr(t), t.shape[0], t.shape[1], rf_interp, rf_deci, gain, mode, _ptr(a), len(a), audio_interp, audio_deci, scale)
    return Block(h, in_dtype, np.float32)


def FmReceiver(taps_per_channel, rf_interp: int, rf_deci: int, audio_taps, audio_interp: int, audio_deci: int,
               gain: float = 1.0, mode: int = ATAN2_EXACT, scale: float = 1.0) -> Block:
    """The N-station FM receiver down to audio (rr_fm_receiver_create): Tee + N x (FftFilter(taps_c) -> RationalResampler ->
    QuadratureDemod -> FftFilterFloat(audio_taps) -> RationalResampler -> MultiplyConst), examples/rtl_fm.rs:381-419 per
    channel, two tile launches per call.  taps_per_channel = [N][ntaps]; audio_taps is shared.  work() returns out with
    shape (N, produced); work_dev() takes N windows of out_cap f32 elements."""
    return _fm_receiver(lib().rr_fm_receiver_create, np.complex64, taps_per_channel, rf_interp, rf_deci, audio_taps,
                        audio_interp, audio_deci, gain, mode, scale)


def FmReceiverU8(taps_per_channel, rf_interp: int, rf_deci: int, audio_taps, audio_interp: int, audio_deci: int,
                 gain: float = 1.0, mode: int = ATAN2_EXACT, scale: float = 1.0) -> Block:
    """RtlSdrDecode -> FmReceiver fused: RTL-SDR bytes in, N f32 audio windows out (windows, consumed and the WAIT_SRC need
    count bytes)."""
    return _fm_receiver(lib().rr_fm_receiver_u8_create, np.uint8, taps_per_channel, rf_interp, rf_deci, audio_taps,
                        audio_interp, audio_deci, gain, mode, scale)


def Hilbert(ntaps: int, wtype: int = WIN_HAMMING, parm: float = 0.0) -> Block:
    return Block(lib().rr_hilbert_create(ntaps, wtype, parm), np.float32, np.complex64)
