/*
 * rustradio_amd.h — C ABI of the MI355X-native rustradio hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point cites the interface of ThomasHabets/rustradio (v0.18.2) it
 * replaces; INTEGRATION.md shows the Rust `impl Block` shim that binds them.
 *
 * One opaque `rr_block` per block instance (the reference's struct fields:
 * taps, carry state).  A handle is not thread-safe but may move between
 * threads (`Block: Send`, src/block.rs:115); it owns a HIP stream and its
 * device buffers, and there is no global mutable state, so N handles can run
 * on N host threads or N GPUs.
 *
 * The library is GPU-only: every entry point that computes fails (NULL /
 * RR_ERR, message in rr_last_error()) when no HIP device is usable.  There is
 * no CPU fallback.
 */
#ifndef RUSTRADIO_AMD_H
#define RUSTRADIO_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 3   /* 3 (round 5): rr_block_tag_rule; zero-copy host windows only for page-aligned ranges (rr_host_register), RR_ZERO_COPY=0.  2 (round 4): rr_dstream_close / _closed / _wait / _id, RR_ROT_REPLAY_DEVICE; rr_build_opts.host_sync_copies removed */

/* Complex<f32>: interleaved [re, im], 8 bytes (src/lib.rs:268-271). */
typedef struct { float re, im; } rr_c32;

typedef struct rr_block rr_block;

/* BlockRet (src/block.rs:12-70).  RR_WAIT_SRC / RR_WAIT_DST are
 * WaitForStream(&self.src, need) / WaitForStream(&self.dst, need). */
enum rr_status {
    RR_AGAIN = 0,
    RR_WAIT_SRC = 1,
    RR_WAIT_DST = 2,
    RR_EOF = 3,
    RR_PENDING = 4,
    RR_ERR = -1
};

/* WindowType (src/window.rs:42-60). */
enum rr_window { RR_WIN_HAMMING = 0, RR_WIN_BLACKMAN = 1, RR_WIN_BLACKMAN_HARRIS = 2, RR_WIN_HAMMING_PARM = 3 };

/* QuadratureDemod atan2 flavour: RR_ATAN2_EXACT = `f32::atan2`
 * (--no-default-features build, src/quadrature_demod.rs:96-109);
 * RR_ATAN2_FAST = `fast_math::atan2` (default Cargo feature, :77-81). */
enum rr_atan2 { RR_ATAN2_EXACT = 0, RR_ATAN2_FAST = 1,
                /* fused-chain constructors only (rr_fm_chain*_create, rr_fm_multi*_create): the chain's demodulator is the
                 * FastFM block (src/quadrature_demod.rs:144-165: one output per resampled sample, two samples of history,
                 * `gain` unused) instead of QuadratureDemod */
                RR_DEMOD_FASTFM = 2 };

/* Rotator evaluation for FirFilter::translate (src/fir.rs:464-473: `sample *= phase; phase *= step` in f32, never
 * renormalised):
 * RR_ROT_REPLAY = DEFAULT.  The reference's sequential f32 recurrence replayed bit for bit, for any stream length.  The
 *                 chain is data-independent, so it is generated AHEAD of the filter on a side stream while the filter
 *                 kernels of the current window run; a call waits only for what the chain has not reached.  It starts
 *                 on the device: one lane walks it from the phase carried in device memory (three packed f32
 *                 instructions per step, 10 ns per output = 100 M outputs/s; no host thread, no PCIe traffic) — enough
 *                 for any graph paced by its source (BASELINE configs[4]: 12.5 M outputs/s).  A block whose calls keep
 *                 arriving before the look-ahead has finished (three in a row: back-to-back batch calls) is given a host
 *                 generator instead: one thread walks the same chain in strict f32 at an x86 core's multiply + add
 *                 latency (2.6 ns per output) from the device chain's current phase into a pinned ring, copied ahead
 *                 into the device ring (8 B per output over PCIe).  The sequential chain bounds such a block either
 *                 way ("sequential_rotator" in bench.py).
 * RR_ROT_REPLAY_DEVICE = the device chain only (never a thread).  RR_ROT_REPLAY_HOST = the host generator from the first
 *                 call.  Bit-identical to each other and to the reference in every case.
 * RR_ROT_MODEL  = opt-in: closed form phase0 * step^m evaluated in f64 from the SAME f32-rounded phase0 / step
 *                 (parallel, as fast as the filter).  NOT parity-faithful for long streams: it differs from the
 *                 recurrence by its accumulated rounding, <= 1e-7 * n after n outputs (measured 1.5e-8 * n:
 *                 tests/test_gpu_edges_fullsize.py::test_rotator_drift_vs_length), i.e. inside the 1e-5 bar only for
 *                 the first ~1e2 (bound) .. 1e5 (measured) outputs of a stream. */
enum rr_rotator { RR_ROT_MODEL = 0, RR_ROT_REPLAY = 1, RR_ROT_REPLAY_DEVICE = 2, RR_ROT_REPLAY_HOST = 3 };

/* ---- library / device ------------------------------------------------------ */
int         rr_abi_version(void);
const char *rr_last_error(void);            /* thread-local message of the last failure */
int         rr_device_count(void);          /* number of visible HIP devices (0 if none) */
int         rr_set_device(int ordinal);     /* device used by blocks created afterwards on this thread */

/* Path-selection overrides for ONE block: rr_next_create_options(&o) applies `o` to the next rr_*_create /
 * rr_dstream_create call made on the calling thread and is cleared when that call returns (thread-local, so
 * handles stay independent and nothing in the process environment changes what a block does).  A zeroed struct =
 * every choice automatic.  Every path stays within the 1e-5 parity bar; the overrides exist so that the parity
 * tests and A/B probes can reach each kernel. */
enum rr_path { RR_PATH_AUTO = 0, RR_PATH_DIRECT = 1, RR_PATH_FFT = 2 };
typedef struct {
    int fir_path;           /* FirFilter / Hilbert>FirFilter: RR_PATH_DIRECT = direct-form kernels only,
                               RR_PATH_FFT = overlap-save tiles for every shape they cover */
    int fir_prune;          /* decimations 4 / 8 / 16: pruned inverse transform, > 0 on, < 0 off */
    int fir_half;           /* other even decimations: half-size inverse, < 0 off */
    int fir_cfg_plus1;      /* direct-form FIR tile shape 0..7, stored + 1 (0 = automatic) */
    int fft_log2f;          /* FftFilter: overlap-save tile of 2^n points, n = 10..14 */
    int fft_no_split;       /* tiles of 8192 / 16384 points as ONE workgroup instead of 2 / 4 sub-transforms */
    int fftfloat_complex;   /* FftFilterFloat: the reference's f32 -> Complex -> FftFilter -> .re inner path */
    int fm_full;            /* fused FM chains and rr_channelizer*_create: full-size inverse transforms for 1:even ratios too
                               (and never the decimate-first tiles) */
    int fm_poly;            /* fused FM chains and rr_channelizer*_create: decimate-first (polyphase) tiles, > 0 wherever
                               supported, < 0 never; 8 / 12: also fixes the multi-channel kernel's waves per workgroup
                               (0 / 1: by predicted cost) */
    int dstream_no_vmm;     /* rr_dstream_create: the copying fallback ring instead of the double mapping */
    int fir_poly;           /* decimating FirFilter<Complex>: decimate-first (polyphase) tiles, > 0 wherever supported, < 0 never */
    int fft_nonfinite_tiles;/* FftFilter / FftFilterFloat: 1 = leave a NaN / Inf input sample's damage on the GPU's tile instead of
                               moving it onto the reference's block of nsamples inputs (no pass behind the tile kernels);
                               3 = do the pass inside the tile kernel's tail (one launch per work(), slower: csrc/blocks.cpp
                               ref_blocks_on); 0 / 2 = the default, a small launch of its own behind every call */
    int host_in_staged;     /* rr_block_work on a page-locked INPUT window: > 0 copy it to device memory first (a copy kernel, 55 GB/s)
                               instead of letting the block's kernels read it in place, < 0 always in place; 0 = the block's default */
    int sync_lanes;         /* rr_symbol_sync_create: streams per wave of the clock kernel, 1 or 64; 0 = by stream count */
    int sync_prof_launch;   /* rr_symbol_sync_create: 1 / 2 / 3 = rr_block_profile times that launch of a push (signs, clock, gather)
                               alone; 0 = the three as one bracket */
    int reserved[1];
} rr_build_opts;
int rr_next_create_options(const rr_build_opts *opts);   /* NULL clears a pending override */

/* ---- tap designers (setup time; host f32, same operation order as the reference) */
float  rr_max_attenuation(int window);                                   /* src/window.rs:67-75 */
int    rr_make_window(int window, float parm, size_t ntaps, float *out); /* src/window.rs:79-185 */
size_t rr_compute_ntaps(float samp_rate, float twidth, int window);      /* src/fir.rs:606-610 */
/* low_pass (src/fir.rs:617-656): returns ntaps, writes min(ntaps, cap) taps; 0 on bad args. */
size_t rr_low_pass(float samp_rate, float cutoff, float twidth, int window, float parm,
                   float *out, size_t cap);
/* low_pass_complex (src/fir.rs:594-604). */
size_t rr_low_pass_complex(float samp_rate, float cutoff, float twidth, int window, float parm,
                           rr_c32 *out, size_t cap);
/* multiband(bands, taps, window) (src/fir.rs:552-590): bands = nbands (low, high) pairs in units of Nyquist,
 * window = ntaps window values; RR_ERR for the reference's None. */
int    rr_multiband(const float *bands, size_t nbands, const float *window, size_t ntaps, rr_c32 *out);
/* hilbert(window) (src/fir.rs:660-680). */
int    rr_hilbert_taps(const float *window, size_t ntaps, float *out);

/* ---- block constructors ------------------------------------------------------ */
/* FirFilter::<Complex>::builder(taps).deci(deci)[.translate(samp_rate, freq)].build(src)
 * (src/fir.rs:303-386, 476-486).  translate != 0 requests frequency translation
 * (freq == 0 disables it, fir.rs:438-440).  NULL on invalid args (the reference asserts).
 * Arithmetic: Fir::filter_n (fir.rs:166-197) in direct form or on overlap-save FFT tiles (plain, decimating store,
 * half-size / pruned inverse, decimate-first), whichever is cheaper for (ntaps, deci) AND the window of the call — the
 * block carries no arithmetic state between calls, so a 512,000-sample ring and a 1e8-sample batch may take different
 * kernels; all within 1e-5 of the reference (rr_fir_fft_tile tells the large-window choice; rr_build_opts forces one). */
rr_block *rr_fir_c32_create(const rr_c32 *taps, size_t ntaps, size_t deci,
                            int translate, float samp_rate, float freq);
/* FirFilter::<Float> (same generic block, src/fir.rs:343-386; long filters on real-stream overlap-save tiles). */
rr_block *rr_fir_f32_create(const float *taps, size_t ntaps, size_t deci);
/* FftFilter::new(src, taps) (src/fft_filter.rs:242-279).  Up to 16383 taps run on LDS-resident overlap-save tiles; longer
 * filters (up to 524,288 taps; the reference has no limit) as overlap-save frames of 2^m >= 2 ntaps points through the
 * any-size transform (plain HBM-streaming passes).  The tile size is internal (rr_fftfilter_dims reports it) and, for long
 * filters, depends on the window of the call; outputs do not depend on it beyond f32 rounding.  A NaN / Inf input sample
 * makes the reference's outputs non-finite — the fft_size outputs from the start of its block of nsamples inputs
 * (src/fft_filter.rs:326-347) — whatever tile ran (a small pass behind the tile kernels of every call; FftFilterFloat too). */
rr_block *rr_fftfilter_create(const rr_c32 *taps, size_t ntaps);
/* FftFilterFloat::new(src, taps) (src/fft_filter.rs:391-426). */
rr_block *rr_fftfilter_float_create(const float *taps, size_t ntaps);
/* RationalResampler::<T>::new(src, interp, deci) for any Copy T of elem_size
 * bytes, elem_size in {1,2,4,8,16} (src/rational_resampler.rs:125-151).
 * NULL (reference: Err) when interp or deci is 0. */
rr_block *rr_resampler_create(size_t interp, size_t deci, size_t elem_size);
/* QuadratureDemod::new(src, gain) (src/quadrature_demod.rs:32-43). */
rr_block *rr_quaddemod_create(float gain, int atan2_mode);
/* RtlSdrDecode::new(src) (src/rtlsdr_decode.rs:9-47): u8 I/Q byte pairs -> Complex,
 * (b - 127) * 0.008; input windows are counted in BYTES, an odd trailing byte is left unconsumed. */
rr_block *rr_rtlsdr_decode_create(void);
/* FftStream::new(src, size) (src/fft_stream.rs:40-117): the forward, unnormalised FFT of every consecutive
 * `size`-sample frame, natural bin order; work(): WAIT_SRC(size) / WAIT_DST(size), else whole frames of
 * min(in, out), RR_AGAIN.  The frame tags (TAG_FRAME, TAG_FRAME_SIZE) are added by the shim from
 * `produced`.  ANY size from 2 to the stream capacity (512,000; rustfft plans any size): one tile kernel up to 16384 = 2^14
 * points and for every size up to 2048 (Bluestein chirp-z on a filter tile), the four-step decomposition for larger powers
 * of two, Bluestein on a power of two M >= 2 size - 1 for everything else. */
rr_block *rr_fftstream_create(size_t size);
/* Fft::from_fft_size(prev, size) (src/fft.rs:19-56): the message (PDU) form — one Vec<Complex> of exactly `size` samples
 * in, its forward FFT out.  The handle is an rr_fftstream_create(size) block; rr_fft_process transforms ONE message held in
 * host memory (n != size: RR_ERR, "FFT expected {size} samples, got {n}" as fft.rs:46-52).  The shim pops the message from
 * its NCReadStream, calls this, pushes the result with the message's tags. */
int rr_fft_process(rr_block *fftstream, const rr_c32 *msg, size_t n, rr_c32 *out);
/* MultiplyConst::<Float|Complex>::new(src, val) (src/multiply_const.rs:6-23) and FastFM::new(src)
 * (src/quadrature_demod.rs:144-165): #[rustradio(sync)] blocks — work() maps min(input, output space)
 * samples and returns WaitForStream(src|dst, 1) (rustradio_macros_code/src/lib.rs:458-515).  Bit-exact. */
rr_block *rr_multiply_const_f32_create(float val);
rr_block *rr_multiply_const_c32_create(float re, float im);
rr_block *rr_fastfm_create(void);
/* AddConst::<Float|Complex>::new(src, val) (src/add_const.rs:51-68): a #[rustradio(sync)] block like MultiplyConst, same
 * protocol, tags kept; out = in + val, one f32 add per component.  Bit-exact. */
rr_block *rr_add_const_f32_create(float val);
rr_block *rr_add_const_c32_create(float re, float im);
/* Hilbert::new(src, ntaps, &window_type) (src/hilbert.rs:38-61); ntaps odd > 1. */
rr_block *rr_hilbert_create(size_t ntaps, int window, float window_parm);
/* Vco::new(src, k) (src/vco.rs:9-37): Float in, Complex out.  Per sample a: phase += k * a in f64, one wrap by 2 pi when the
 * phase leaves [-2 pi, 2 pi], output Complex::new(phase.sin() as f32, phase.cos() as f32) — re is the SINE and im the cosine,
 * i.e. the stream is j e^(-j phase) and a quadrature demodulator sees -k * a.  k_bits = the f64 `k` as its IEEE-754 binary64
 * bit pattern (f64::to_bits), so that a k computed in f64 arrives exactly; any finite or non-finite k is accepted.
 * #[rustradio(sync)]: work() maps min(input, output space) samples, WaitForStream(src|dst, 1) (rustradio_macros_code/src/lib.rs:
 * 458-515); tags forwarded position for position.  The running sum is a tiled f64 scan; the phase carried between calls stays
 * in device memory.  Which multiple of 2 pi the phase holds is not observable, so outputs agree with the reference's within
 * 2^-25 + n * 2^-48 per component after n samples (|k * a| <= 2 pi), not bit for bit.  From the first NaN / +-Inf input sample
 * on, both components of EVERY later output are NaN, in that call and all later ones (Inf - 2 pi = Inf, sin(Inf) = NaN); the
 * outputs before it are untouched. */
rr_block *rr_vco_create(unsigned long long k_bits);
/* ComplexToMag2::new(src) (src/complex_to_mag2.rs:8-21): Complex in, f32 out, re*re + im*im with the reference's three
 * f32 roundings (num-complex norm_sqr, no FMA).  #[rustradio(sync)].  Bit-exact.  Tags: RR_TAGS_FORWARD, 1. */
rr_block *rr_complex_to_mag2_create(void);
/* The first Map of examples/airspy_am_decode.rs ("AirSPY to Complex"): input elements are 4 bytes, a little-endian u32 with I in
 * the low 16 bits and Q in the high 16, each an i16; out = Complex(f32(i) / 1000.0, f32(q) / 1000.0), two true IEEE f32 divisions
 * (num-complex divides each component; no reciprocal).  #[rustradio(sync)], the protocol of rr_complex_to_mag2; input windows
 * count u32 elements.  Bit-exact.  Tags: RR_TAGS_FORWARD, 1. */
rr_block *rr_airspy_decode_create(void);

/* SinglePoleIirFilter::<Float|Complex>::new(src, alpha) (src/single_pole_iir_filter.rs:11-93): elem_size 4 or 8 (Complex:
 * re and im are two independent recurrences).  y = x*alpha + y_prev*(1 - alpha), y_prev = 0 at the start, carried across calls
 * in device memory.  NULL + rr_last_error ("alpha out of range") unless 0 <= alpha <= 1 (NaN included: reference returns
 * None).  #[rustradio(sync)]; tags RR_TAGS_FORWARD, 1.  Accuracy and non-finite samples: below. */
rr_block *rr_single_pole_iir_create(float alpha, size_t elem_size);
/* Accuracy of the two scan blocks (this one and rr_burst_detector_create).  With a = alpha and b = fl32(1.0f - alpha), the
 * reference's two f32 fields, widened to f64, and t[n] = a x[n] + b t[n-1] in real arithmetic: the recurrence runs as a tiled
 * scan in f64 with ONE cast to f32 at the store, so
 *   |out[n] - t[n]| <= 2^-24 |t[n]| + 2^-53 X (64 + 4 / alpha),   X = max |x| over the stream so far,
 * closer to t than the reference's own f32 fold (whose drift is up to 2.01 * 2^-24 X / alpha); not bit-equal to it.  alpha 0
 * gives exactly 0.0f, alpha 1 gives x bit for bit.  Non-finite samples: a NaN sample makes its own output and EVERY later one
 * NaN, in that call and in all later calls (the reference's prev_output stays NaN); the outputs before it are untouched.  A
 * +-Inf sample makes every output from there on non-finite; whether a given one is Inf or NaN is not pinned (Inf times an
 * underflowed power of b is NaN where the reference may still hold Inf). */

/* Graph-level fusion of three reference blocks wired as in examples/rtl_fm.rs:381-419:
 *   FftFilter::new(src, taps) -> RationalResampler::new(_, interp, deci) -> QuadratureDemod::new(_, gain)
 * as ONE block (Complex in, f32 out) whose whole-stream output equals that of the three blocks in
 * sequence (src/fft_filter.rs:290-354, src/rational_resampler.rs:155-206,
 * src/quadrature_demod.rs:46-113); the filtered and resampled streams never reach HBM.
 * work(): WAIT_DST(n) when the next filter block's outputs do not fit, else consumes like
 * FftFilter (whole pending block) and WAIT_SRC(nsamples - pending).
 * The output stream must be able to hold one filter block's worth of demodulated samples,
 * ceil(nsamples * interp / deci) (the three separate blocks need only `nsamples` Complex slots in THEIR rings):
 * with the reference's 4,096,000-byte streams that is any ratio up to interp/deci ~ 60 at 16384-point blocks; a
 * smaller output window returns WAIT_DST(n) forever — use the three blocks there.
 * No tap-count limit (the reference has none, src/fft_filter.rs:36-42): up to 16383 taps the chain is one kernel per call;
 * beyond that — or for a decimation larger than a tile — the SAME constructor returns the unfused composition of the three
 * GPU blocks behind the one handle (device-resident intermediates, one work() call, same whole-stream output).
 * atan2_mode = RR_DEMOD_FASTFM puts FastFM (src/quadrature_demod.rs:144-165) in the demodulator's place: one output per
 * resampled sample, bit-exact against FftFilter -> RationalResampler -> FastFM (composition; `gain` unused). */
rr_block *rr_fm_chain_create(const rr_c32 *taps, size_t ntaps, size_t interp, size_t deci,
                             float gain, int atan2_mode);

/* Graph-level fusion of FirFilter::<Complex>::builder(fir_taps).build(src) (deci 1, src/fir.rs:303-386) ->
 * FftFilter::new(_, fft_taps) (src/fft_filter.rs:242-279) — the north star's "127-tap FIR + 1024-pt FftFilter chain" —
 * as ONE convolution with the composite taps fir_taps (*) fft_taps (formed in f64, rounded once).  Whole-stream output
 * equals the two blocks in sequence to f32 rounding, INCLUDING the start of the stream, where FftFilter sees zero
 * history rather than a warm FIR: those fft_ntaps - 1 outputs are recomputed from the two-stage definition.
 * work(): WAIT_DST(nsamples) when a block of the FftFilter stage does not fit (fft_filter.rs:294-303), WAIT_SRC(fir_ntaps)
 * below the FIR's minimum (fir.rs:498-501); otherwise consumes len - (fir_ntaps - 1) samples like the FIR (its history
 * stays in the caller's ring, fir.rs:537), emits whole blocks of nsamples = fft_size(fft_ntaps) - fft_ntaps and returns
 * WAIT_SRC(nsamples - pending + fir_ntaps - 1) / WAIT_DST(nsamples).  Non-finite input samples: the reference's set — the
 * FIR outputs whose fir_ntaps windows hold one, and through them the FftFilter stage's whole blocks (see rr_fftfilter_create). */
rr_block *rr_fir_fftfilter_create(const rr_c32 *fir_taps, size_t fir_ntaps, const rr_c32 *fft_taps, size_t fft_ntaps);
/* ... followed by RationalResampler(interp, deci) -> QuadratureDemod(gain): the metric's whole chain
 * FIR + FftFilter + Resampler + QuadDemod as one kernel (rr_fm_chain_create with the composite filter and the same
 * head fix).  Complex in, f32 out. */
rr_block *rr_fir_fm_chain_create(const rr_c32 *fir_taps, size_t fir_ntaps, const rr_c32 *fft_taps, size_t fft_ntaps,
                                 size_t interp, size_t deci, float gain, int atan2_mode);

/* The same with RtlSdrDecode::new(src) (src/rtlsdr_decode.rs:9-47) fused in front, the receive chain of
 * examples/rtl_fm.rs:328-419 from the RTL-SDR byte stream onwards: u8 in, f32 out, 2 B instead of 8 B
 * read per sample.  Input windows, `consumed` and the WAIT_SRC `need` count BYTES; an odd trailing
 * byte stays unconsumed (rtlsdr_decode.rs:23).  Whole-stream output == RtlSdrDecode -> rr_fm_chain. */
rr_block *rr_fm_chain_u8_create(const rr_c32 *taps, size_t ntaps, size_t interp, size_t deci,
                                float gain, int atan2_mode);

/* Graph-level fusion of the audio stage of examples/rtl_fm.rs:398-418:
 *   FftFilterFloat::new(src, taps) -> RationalResampler::new(_, interp, deci) -> MultiplyConst::new(_, scale)
 * (src/fft_filter.rs:365-491, src/rational_resampler.rs:125-206, src/multiply_const.rs:6-23) as ONE real-valued kernel:
 * f32 in, f32 out; whole-stream output equals the three blocks in sequence.  work() like rr_fm_chain_create: WAIT_DST(n)
 * when the next filter block's resampled samples do not fit, else consumes like FftFilter (whole pending block) and
 * WAIT_SRC(nsamples - pending).  Up to 3584 taps one kernel per call; longer filters run as the unfused composition of
 * the three GPU blocks behind the same handle (no tap-count limit, as in the reference). */
rr_block *rr_audio_chain_create(const float *taps, size_t ntaps, size_t interp, size_t deci, float scale);

/* Graph-level fusion of the modulator of examples/fm_tx.rs:84-91:
 *   RationalResampler::new(src, interp, deci) -> Vco::new(_, k)
 * (src/rational_resampler.rs:125-206, src/vco.rs:9-37) as ONE block, f32 in, Complex out: the interpolated f32 stream never
 * reaches HBM, the phase accumulates once per OUTPUT sample.  k_bits as rr_vco_create; re = sin, im = cos.  work() is
 * rr_resampler_create(interp, deci, _)'s call for call — same status, consumed, produced and need on windows of the same
 * lengths, the pending sample across a full output window and eof = !pending && src_eof included; the ratio is gcd-reduced;
 * NULL (reference: Err) when interp or deci is 0.  Tags are dropped (the resampler's rule).  Accuracy and non-finite samples
 * as rr_vco_create, counted in output samples. */
rr_block *rr_fm_tx_create(size_t interp, size_t deci, unsigned long long k_bits);

/* Graph-level fusion of the burst path of examples/burst_saver.rs:111-123:
 *   ComplexToMag2 -> SinglePoleIirFilter(alpha) -> the comparison of BurstTagger(threshold) (src/burst_tagger.rs:68-85)
 * Complex in; f32 out = the filtered power (what SinglePoleIirFilter delivers to BurstTagger's trigger input); sync protocol.
 * Besides, every call records the positions i (relative to the call's window) at which cur(i) = (out[i] > threshold) differs
 * from cur(i-1); cur(-1) is the previous call's last value, false at the start of the stream: exactly where BurstTagger
 * pushes Tag(pos, tag, Bool(cur)).  alpha as rr_single_pole_iir_create.  The envelope is bit-identical to
 * rr_complex_to_mag2 -> rr_single_pole_iir on windows of the same lengths, and cur(i) is decided on the f32 actually stored.
 * Accuracy and non-finite samples as rr_single_pole_iir_create; edges after a +-Inf sample are unspecified, a NaN envelope is
 * never above the threshold, and a NaN threshold yields no edges. */
rr_block *rr_burst_detector_create(float alpha, float threshold);

/* The edges of the block's most recent work call, ascending.  Waits for that call (as rr_block_sync), writes the first
 * min(*total, cap) of them: pos[j] window-relative, val[j] = 1 (rose above threshold) / 0.  *total = how many there were;
 * a call that moved no samples has none.  No edge is ever dropped on the device: its list holds one entry per sample of the
 * largest window seen.  RR_ERR for a handle that is not a burst detector. */
int rr_burst_edges(rr_block *b, size_t *pos, unsigned char *val, size_t cap, size_t *total);

/* The bit-level sync blocks every data receiver of the reference runs after its symbol clock
 * (examples/ax25-9600-rx.rs:195-204, examples/il2p-1200-rx.rs:118-126).  All are #[rustradio(sync)] / sync_tag: n = min(in_len,
 * out_cap) samples per call, tags RR_TAGS_FORWARD, 1.  All are exact in integers: bit-identical to the reference, whatever the
 * split of the stream into calls; the state between calls stays on the device.  One kernel launch per call.
 * The u8-input blocks are specified for inputs 0 and 1 only (the reference's Descrambler panics on anything else,
 * src/descrambler.rs:35; here only the lowest bit of a byte is looked at).
 *
 * BinarySlicer::new(src) (src/binary_slicer.rs:8-20): f32 in, u8 out, out = x > 0.0, so NaN, -0.0, 0.0 and -Inf give 0. */
rr_block *rr_binary_slicer_create(void);
/* NrziDecode::new(src) (src/nrzi.rs:25-42): u8 in, u8 out, out[n] = 1 ^ in[n] ^ in[n-1], in[-1] = 0 at the start of the stream. */
rr_block *rr_nrzi_decode_create(void);
/* Descrambler::new(src, mask, seed, len) (src/descrambler.rs:13-39,50-93): u8 in, u8 out, the self-synchronising LFSR
 * out = parity(shift_reg & mask) ^ in, shift_reg = shift_reg >> 1 | in << len.  G3RUH is (0x21, 0, 16).  NULL + rr_last_error:
 * "descrambler length out of range" for len >= 64 (the reference asserts), "seed wider than the register" for a seed with a
 * bit above bit len (a deviation: the reference would let such bits shift down into the mask; no example has one).  Mask bits
 * above bit len never meet a set bit and are ignored. */
rr_block *rr_descrambler_create(unsigned long long mask, unsigned long long seed, unsigned len);
/* CorrelateAccessCodeTag::new(src, code, tag, allowed_diffs) (src/correlate_access_code.rs:58-119): u8 in, the same u8 out; every
 * position whose last code_len bits differ from the code in at most allowed_diffs places is recorded for rr_bit_tags, once
 * code_len bits of the stream have been seen.  The code travels packed: bit k of `code` is code[k], code[0] (the oldest bit)
 * in bit 0.  NULL + rr_last_error: "access code must be nonempty" (the reference's assert), "access code longer than 64 bits". */
rr_block *rr_correlate_access_code_tag_create(unsigned long long code, unsigned code_len, size_t allowed_diffs);
/* Graph-level fusion of the chain above: BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler(mask, seed, len)] ->
 * [CorrelateAccessCodeTag(code, allowed_diffs)], the stages in this order, f32 soft symbols in, u8 bits after the last enabled
 * stage out.  flags: which optional stages run; mask, seed, len are read only with RR_BITS_DESCRAMBLE; code_len == 0: no
 * correlator.  Errors as the single blocks, and "unknown bit decoder flags".  Output and tags are bit-identical to the
 * separate blocks in sequence. */
enum { RR_BITS_INVERT = 1, RR_BITS_NRZI = 2, RR_BITS_DESCRAMBLE = 4 };
rr_block *rr_bit_decoder_create(int flags, unsigned long long mask, unsigned long long seed, unsigned len,
                                unsigned long long code, unsigned code_len, size_t allowed_diffs);
/* The sync-word tags of the block's most recent work call, ascending: where process_sync_tags pushes Tag(pos, tag, U64(diffs))
 * (src/correlate_access_code.rs:93-118).  Waits for that call (as rr_block_sync), writes the first min(*total, cap) of them:
 * pos[j] window-relative, diffs[j] the number of differing bits.  *total = how many there were; pos == NULL with cap == 0
 * only counts; a call that moved no samples has none.  No tag is ever dropped on the device: its list holds one entry per
 * sample of the largest window seen.  RR_ERR for a handle without a correlator stage. */
int rr_bit_tags(rr_block *b, size_t *pos, unsigned char *diffs, size_t cap, size_t *total);

/* Wpcr::new(src) / WpcrBuilder::samp_rate (src/wpcr.rs:84-128): whole-packet clock recovery, the symbol clock in front of the
 * bit-level blocks above (examples/ax25-1200-wpcr.rs, ax25-9600-wpcr.rs, g3ruh.rs).  A PDU-form block like rr_fft_process, not a
 * stream block: rr_block_work on the handle is an error.  samp_rate is NaN when not set.  One call takes a BATCH of disjoint
 * bursts inside one f32 sample buffer; per burst x[0 .. n), N = n - 1, with its own `mid` (the reference hard-wires 0.0, :138):
 *   1. n < 4: dropped (the reference's None, :131-133).
 *   2. s[i] = x[i] > mid (NaN: 0); d[i] = (s[i] - s[i+1])^2, i < N: 0 / 1 and finite whatever the samples are (:141-149).
 *   3. X = DFT_N(d), forward, unnormalised, bins k < N / 2; mag[k] = sqrt(re^2 + im^2) in f32 (:153-156, :222).
 *   4. find_best_bin (:217-239): thresh = 0.8f max(mag[2 .. N/2)); bin = the first k >= 2 with k + 1 < N / 2, mag[k] > thresh
 *      and mag[k] > mag[k+1]; none (every N / 2 <= 3, every burst without a crossing, a NaN mid): dropped.
 *   5. f = (float)bin / (float)n (:165; symbols per sample, < 0.5); t = 0.5f + atan2f(im, re) / (float)(2 pi);
 *      p0 = t > 0.5f ? t : t + 1.0f, in (0.5, 1.5] (:166-169).
 *   6. Symbols.  The reference runs `if phase >= 1 { phase -= 1; push(x[i]) }; phase += f` per sample in f32 (:180-186).  This
 *      block evaluates the same clock WITHOUT the accumulator's drift: with P(i) = p0 + i f in exact arithmetic on the two f32
 *      values (64-bit integers on the device), sample i is taken iff floor(P(i)) > floor(P(i-1)) (sample 0 iff p0 >= 1) and
 *      becomes symbol floor(P(i)) - 1; nsyms = floor(P(n-1)); the `phase` tag is fl32(P(n) - nsyms).  NOT bit-equal to the
 *      reference: its f32 phase is off the exact one by at most i 2^-24 after i additions, so its picks differ from this
 *      block's only where P(i) or P(i-1) lies within (i + 1) 2^-24 of an integer (there it takes the neighbouring sample), and
 *      its phase tag differs by at most n 2^-24.  The same stance as rr_vco_create and the scan blocks: closer to the exact
 *      recurrence than the reference.
 *   7. A symbol is x[i] - mid, one f32 rounding: what Midpointer (:75-78) would have put into the burst, and x > mid is what
 *      Wpcr would have seen behind it — a caller that computes Midpointer's offset passes it as `mid` instead of rewriting
 *      the burst.  mid == NULL means 0 for every burst: the symbols are the samples bit for bit (NaN and +-Inf included).
 *   8. Tags (:187-194): sps = f, phase as above, frequency = f * samp_rate in f32 (NaN without a sample rate).
 * Accuracy of the spectrum the decision is taken on.  With C = the number of crossings of the burst and X the exact DFT,
 *   |X_gpu[k] - X[k]| <= C (pi 2^-23 + e_phasor) + depth 2^-24 C,   e_phasor = pi 2^-23 + 2 e_sincos + 3 2^-24, e_sincos = 2^-21,
 *   depth = 20, about 3.1e-6 C:
 * j k mod N is reduced exactly in integers and a phase is rounded to f32 ONCE (2 r / N in [0, 2), error 2^-23, times pi);
 * e_sincos bounds sincospif's error on (cos, sin) as a vector.  One bin in four takes its phasors from sincospif directly; the
 * other three multiply them by a second such phasor (the step of 256, 512 or 768 bins) in f32, which doubles the error of one
 * and adds 3 2^-24 for the product: that is e_phasor.  The terms are summed in f32 in groups of 16 and the groups in f64 (whose
 * own error is below 2^-34 C), so `depth` counts 15 additions, the cast of the f64 sum and the four roundings of
 * norm_sqr().sqrt().  The bound does not depend on N.  p0 follows within bound / |X[bin]| / (2 pi) + 3 2^-24, modulo 1.  Whatever the input (pure noise included),
 * `bin` is find_best_bin applied to the block's OWN f32 magnitudes (rr_debug_wpcr_spectrum), and the symbols, nsyms and phase
 * are exactly those of step 6 run from the REPORTED phase0 and sps. */
typedef struct {
    int ok;                 /* 0: the reference's None (the other fields are 0) */
    unsigned bin;
    float sps, phase0;      /* f and p0 of step 5 */
    float phase, frequency; /* the tag values of step 8 */
    size_t nsyms;
} rr_wpcr_result;
rr_block *rr_wpcr_create(float samp_rate);
/* Device pointers d_samples (n_total f32) and d_syms (n_total f32, not overlapping d_samples); enqueued on hip_stream (used as
 * given, like rr_block_work_dev) and returns without waiting for the kernels.  starts, lens and mid (NULL: 0) are HOST arrays
 * of nbursts entries, read before the call returns (not const-qualified only so that every binding's type map has them).
 * Burst b is d_samples[starts[b] .. starts[b] + lens[b]); its symbols are written to d_syms[starts[b] ..), the same geometry as
 * the input (nsyms <= n / 2 + 1 < n always fits: no offsets to scan, no capacity to run out of); the rest of d_syms is left
 * alone.  The ranges must be ascending, disjoint and inside n_total, else RR_ERR with rr_last_error "bursts overlap" /
 * "burst outside the buffer"; lens[b] may be anything up to the stream capacity in samples (512,000), longer: RR_ERR ("burst
 * longer than 512000 samples").  An error launches nothing.  nbursts == 0 launches nothing.  Four kernel launches per call,
 * whatever the number and the lengths of the bursts. */
int rr_wpcr_process_dev(rr_block *b, const void *d_samples, size_t n_total, size_t *starts, size_t *lens, const float *mid,
                        size_t nbursts, void *d_syms, void *hip_stream);
/* The same with host pointers: copies the samples down, runs, copies the symbols back and waits.  syms (n_total f32) receives
 * burst b's symbols at syms[starts[b] ..) and zeros everywhere else between the first burst's start and the last burst's end. */
int rr_wpcr_process(rr_block *b, const float *samples, size_t n_total, size_t *starts, size_t *lens, const float *mid,
                    size_t nbursts, float *syms);
/* One record per burst of the most recent process call, in burst order.  Waits for that call (as rr_burst_edges does), writes
 * the first min(*total, cap) records; *total = the call's nbursts; res == NULL with cap == 0 only counts. */
int rr_wpcr_results(rr_block *b, rr_wpcr_result *res, size_t cap, size_t *total);

/* BurstTagger::new(data, trigger, threshold, tag) (src/burst_tagger.rs:37-85) -> StreamToPdu::new(_, tag, max_size, tail)
 * (src/stream_to_pdu.rs:88-280) -> optionally Midpointer (src/wpcr.rs:44-82) behind one handle: the middle of the burst
 * receivers (examples/ax25-9600-wpcr.rs:103-139, ax25-1200-wpcr.rs, g3ruh.rs:216-219) between rr_burst_detector / rr_quaddemod
 * and rr_wpcr.  f32 data and an f32 trigger in, one window of both per push; a PDU-forming block like rr_wpcr: rr_block_work on
 * the handle is an error.
 *   Edges.  cur(i) = trigger[i] > threshold (a NaN sample is not above; a NaN threshold gives no edges); an edge lies where
 *     cur(i) != cur(i-1), cur(-1) being the previous push's last value and false at the start of the stream: what
 *     rr_burst_detector reports.  Edges alternate strictly and the first one rises.
 *   Bursts.  The PDUs of a stream are exactly those StreamToPdu pushes when fed BurstTagger's tags, whatever the split of the
 *     stream into pushes.  With the rising edges r_j, their falling edges f_j, L = f_j - r_j and free = 0 at the start: a rising
 *     edge with r_j < free is ignored together with its falling edge; an accepted one with L + tail <= max_size yields the PDU
 *     [r_j, f_j + tail) and sets free = f_j + tail; any other accepted one yields nothing and sets free = r_j + max_size + 1.
 *     A PDU is reported by the push that brings its last sample (and its falling edge); a burst still open is carried.
 *   Arena.  The PDUs completed by a push lie ascending and disjoint in ONE device buffer (rr_pdu_arena_dev), a burst begun in an
 *     earlier push whole: the geometry rr_wpcr_process_dev takes.  The block owns the carry (at most max_size samples, the two
 *     arenas of alternate pushes); the caller keeps no old windows.
 *   Midpointer (flags & RR_PDU_MIDPOINT), for all PDUs of the push at once: mean = fl32(S / len) with S summed in f64 (a
 *     deviation: the reference sums in f32 in order; this is closer to the exact mean); nlow = the samples with !(x > mean);
 *     in the total order of f32::total_cmp, low = the element of rank nlow / 2 and high = the element of rank
 *     nlow + (len - nlow) / 2 (the reference's two medians: without a NaN the !(x > mean) side is a prefix of the sorted burst);
 *     mid = low + (high - low) / 2.0f in f32.  ok = 0 (the reference pushes nothing) when the mean is NaN — then nlow = len —
 *     or nlow is 0 or len; mid is 0 then.  The samples are not rewritten: rr_wpcr subtracts mid itself.
 * NULL + rr_last_error: "max_size beyond 512000 samples" (a deviation: the reference has no limit, but Wpcr takes no longer
 * burst), "unknown stream_to_pdu flags"; both are said before any device is touched. */
enum { RR_PDU_MIDPOINT = 1 };
typedef struct {
    size_t start, len;            /* the burst is arena[start .. start + len) */
    unsigned long long stream_pos;/* absolute position of its first sample in the data stream */
    int ok;                       /* 0: Midpointer pushes nothing for this burst (NaN mean, or one side empty) */
    float mean, mid;              /* Midpointer's mean and offset; 0 without RR_PDU_MIDPOINT */
    size_t nlow;                  /* samples with !(x > mean) */
} rr_pdu_record;
rr_block *rr_stream_to_pdu_create(float threshold, size_t max_size, size_t tail, int flags);
/* One window: n samples of data and of trigger (device pointers), n <= 1,024,000 (longer: RR_ERR).  Enqueued on hip_stream
 * (used as given) and returns without waiting; 5 + ceil(log2(n / 2 + 1)) small launches whatever the trigger holds, one more
 * with RR_PDU_MIDPOINT.  n == 0 launches nothing, reports no PDUs and leaves the state alone. */
int rr_stream_to_pdu_push_dev(rr_block *b, const void *d_data, const void *d_trigger, size_t n, void *hip_stream);
/* The same with host pointers: copies both down, runs and waits. */
int rr_stream_to_pdu_push(rr_block *b, const float *data, const float *trigger, size_t n);
/* The PDUs the most recent push completed, ascending.  Waits for it, writes the first min(*total, cap) records; rec == NULL with
 * cap == 0 only counts (the contract of rr_wpcr_results). */
int rr_pdu_records(rr_block *b, rr_pdu_record *rec, size_t cap, size_t *total);
/* The edges of the most recent push, ascending: pos[j] window-relative, val[j] = cur (1: rising) — the contract of
 * rr_burst_edges, and the same list when fed rr_burst_detector's output and threshold. */
int rr_pdu_edges(rr_block *b, size_t *pos, unsigned char *val, size_t cap, size_t *total);
/* The arena of the most recent push (device memory, *n_total elements of the handle's type: max_size + n); valid until the next push.  NULL, *n_total = 0
 * before the first push and after a push of no samples. */
const void *rr_pdu_arena_dev(rr_block *b, size_t *n_total);
/* The samples of PDU idx of the most recent push, the first min(len, cap) of them, to the host. */
int rr_pdu_fetch(rr_block *b, size_t idx, float *out, size_t cap);
/* Midpointer -> Wpcr over the PDUs of the most recent push of `pdus`: waits for that push, takes its records with ok != 0 (all of
 * them without RR_PDU_MIDPOINT) and calls rr_wpcr_process_dev on the arena with their `mid` (NULL without RR_PDU_MIDPOINT).
 * d_syms holds the arena's n_total floats.  rr_wpcr_results then has one record per such PDU, in order. */
int rr_wpcr_process_pdus(rr_block *wpcr, rr_block *pdus, void *d_syms, void *hip_stream);
/* StreamToPdu<Complex> (the reference block is generic over T: Sample): the same f32 trigger, edges, closed form, records and
 * carried state as rr_stream_to_pdu_create; the data, the arena and the carried open burst are rr_c32.  No flags: Midpointer is a
 * block over Vec<Float>.  rr_stream_to_pdu_push_dev, rr_pdu_records, rr_pdu_edges and rr_pdu_arena_dev (*n_total in rr_c32) serve
 * both kinds of handle; rr_pdu_fetch on a Complex handle, rr_pdu_fetch_c32 and rr_stream_to_pdu_push_c32 on an f32 handle and
 * rr_wpcr_process_pdus on a Complex handle ("wpcr: the PDUs are not f32") are RR_ERR.  The payload is copied bit for bit.
 * NULL + rr_last_error: "max_size beyond 512000 samples", before any device is touched. */
rr_block *rr_stream_to_pdu_c32_create(float threshold, size_t max_size, size_t tail);
int rr_stream_to_pdu_push_c32(rr_block *b, const rr_c32 *data, const float *trigger, size_t n);
int rr_pdu_fetch_c32(rr_block *b, size_t idx, rr_c32 *out, size_t cap);

/* Delay::new(src, delay) (src/delay.rs:25-111) for elements of 1, 4 or 8 bytes, a stream block (rr_block_work /
 * rr_block_work_dev): output position p of the whole stream is T::default() (all zero bytes) for p < delay and input sample
 * p - delay behind that, bit for bit.  One call emits min(remaining delay, out_cap) zeros, then copies min(in_len, the space left)
 * samples — the loop of one work() of the reference — in one launch; consumed and produced depend on lengths only and are final
 * on return.  RR_WAIT_DST when no output space is left (out_cap == 0 included), else RR_WAIT_SRC (nothing left to delay and no
 * input left); need = 1.  rr_block_eof: src_eof and the delay spent (delay.rs:56-60).  Tags: RR_TAGS_SHIFT, delay.
 * Deviations: set_delay is not offered (the reference's own test of a mid-stream change is disabled as "TODO: fix"), and the
 * delay is capped.  NULL + rr_last_error, before any device is touched: "unsupported element size",
 * "delay: more than 1,024,000 samples". */
rr_block *rr_delay_create(size_t delay, size_t elem_size);

/* The sample-rate path of examples/burst_saver.rs:111-131 behind one handle: Tee -> [ComplexToMag2 -> SinglePoleIirFilter(alpha)]
 * and [Delay(delay)] -> BurstTagger(threshold) -> StreamToPdu<Complex>(max_size, tail).  Complex in; PDU records and a Complex
 * arena out.  A batch block: rr_block_work on the handle is an error.  For pushed windows x_0, x_1, ..:
 *   the envelope e and cur(i) = e[i] > threshold are those of rr_burst_detector_create(alpha, threshold) fed the same windows
 *     (the same f64 scan, the same stored f32), so rr_pdu_edges is that handle's rr_burst_edges;
 *   the data stream is d[p] = x[p - delay] for p >= delay and 0 + 0i in front (Delay<Complex>), bit for bit;
 *   the PDUs are those of rr_stream_to_pdu_c32_create(threshold, max_size, tail) pushed (d, e) over the same windows: the same
 *     records (ok = 1, mean = mid = 0), arena geometry (max_size + n elements) and lifetime (until the next push).
 * stream_pos counts positions of the DELAYED stream (the tags sit on Delay's output): stream_pos - delay is the input position of
 * the PDU's first sample, and a PDU that begins before position `delay` starts with Delay's zeros.  A NaN input sample makes the
 * envelope NaN for good (rr_single_pole_iir_create's rule) and a NaN envelope is never above the threshold: no further edges.
 * rr_pdu_records, rr_pdu_edges, rr_pdu_arena_dev and rr_pdu_fetch_c32 take the handle under their own contracts.
 * One stream per handle (N channels of a channelizer: N handles fed its rows); no back-pressure: a push takes the whole window.
 * NULL + rr_last_error, before any device is touched: "alpha out of range", "max_size beyond 512000 samples",
 * "delay: more than 1,024,000 samples". */
rr_block *rr_burst_saver_create(float alpha, float threshold, size_t delay, size_t max_size, size_t tail);
/* One window of n <= 1,024,000 Complex samples (device pointer; longer, or NULL with n > 0: RR_ERR before anything is enqueued).
 * d_env: NULL, or n f32 that receive the envelope (rr_burst_detector's output).  Enqueued on hip_stream (used as given), returns
 * without waiting and decides nothing on the host from device data; the launch count depends on n alone
 * (rr_burst_saver_dims).  n == 0 launches nothing, reports no PDUs and leaves every state alone. */
int rr_burst_saver_push_dev(rr_block *b, const void *d_in, size_t n, void *d_env, void *hip_stream);
/* The same with host pointers: copies the window down, runs, waits, and copies the envelope back when env is given. */
int rr_burst_saver_push(rr_block *b, const rr_c32 *in, size_t n, float *env);
/* *tile = the samples of one tile of the scan and of the edge kernels (2048); *launches = the kernel launches of a push of n
 * samples. */
int rr_burst_saver_dims(const rr_block *b, size_t n, size_t *tile, size_t *launches);
/* PduToStream (src/pdu_to_stream.rs:57-101) over the most recent process call of `wpcr`: the symbols of every burst with ok
 * and nsyms > 0, in burst order, back to back in d_out (device, out_cap f32), by ONE gather launch on hip_stream (the offsets
 * come from the host's copy of the results; the call waits for them).  *produced = symbols written; pdu_start[j] / pdu_len[j]
 * (the first min(*npdus, cap) of them; NULL with cap == 0: none) = where packed PDU j begins in d_out and how long it is —
 * the positions of PduToStream's `start` / `end` tags, the latter carrying U64(len).  out_cap too small: RR_ERR ("output
 * shorter than the packed symbols"), nothing launched. */
int rr_wpcr_pack_dev(rr_block *wpcr, const void *d_syms, void *d_out, size_t out_cap, size_t *produced,
                     size_t *pdu_start, size_t *pdu_len, size_t cap, size_t *npdus, void *hip_stream);

/* The bit-level blocks of the packet TRANSMITTERS (examples/g3ruh.rs:250-267, examples/bell202.rs:160-176), the mirror image of
 * the sync blocks above: u8 in, u8 out, #[rustradio(sync)]: n = min(in_len, out_cap) samples per call, tags RR_TAGS_FORWARD, 1.
 * Exact in integers: bit-identical to the reference whatever the split of the stream into calls; the state between calls stays
 * on the device.  Only the lowest bit of an input byte is read.  Three small launches per call.
 *
 * NrziEncode::new(src) (src/nrzi.rs:52-69): out[n] = out[n-1] ^ (in[n] == 0), out[-1] = 0 at the start of the stream. */
rr_block *rr_nrzi_encode_create(void);
/* Scrambler::g3ruh(src) (src/descrambler.rs:41-47, 95-123): with s[n] = in[n] ^ s[n-12] ^ s[n-17] and every s before the stream
 * 0, out[n] = s[n-17].  So the first 17 outputs of a stream are 0, n input bits give n output bits, and the last 17 bits stay in
 * the register until more input comes (the reference's behaviour, kept). */
rr_block *rr_scrambler_g3ruh_create(void);

/* FcsAdder (src/hdlc_framer.rs:28-42) -> HdlcFramer (hdlc_encode, src/hdlc_framer.rs:60-86) -> PduToStream<u8>
 * (src/pdu_to_stream.rs:57-101) -> [Scrambler::g3ruh] -> [NrziEncode] -> [Map(bit ? hi : lo)] behind one handle: everything of the
 * transmit chains in front of RationalResampler, in the order of examples/g3ruh.rs.  (RationalResampler copies samples and never
 * filters, src/rational_resampler.rs:183-197, so the Map commutes with it: the f32 levels at the bit rate are what rr_fm_tx
 * takes.)  A PDU-form block like rr_wpcr: rr_block_work on the handle is an error.  One push takes a BATCH of packets inside one
 * byte buffer and frames them in array order; every stage is bit-identical to the reference's block:
 *   FcsAdder (RR_FRAME_FCS): CRC-16/X.25 (calc_crc, src/hdlc_deframer.rs:309-315) appended low byte first; rec.fcs holds it
 *     (0 without the flag).
 *   HdlcFramer: 20 flags 01111110, the bytes LSB first with a 0 stuffed behind every fifth consecutive 1, 20 flags.  The count
 *     of ones starts at 0 for every packet and is reset by a stuffed bit; five ones that end the packet are still followed by
 *     their 0; an empty packet without FCS is 320 bits of flags.  rec.stuffed = the stuffed bits.
 *   PduToStream: the frames lie back to back in d_out; rec.start / rec.len are the positions of its `start` tag and of the
 *     U64(len) it carries.  The sum of the lengths is *produced.
 *   Scrambler::g3ruh (RR_FRAME_G3RUH), then NrziEncode (RR_FRAME_NRZI), both as the sync blocks above over the concatenated
 *     stream: the register and the level are carried from push to push, so the output of a stream of packets is the same
 *     whatever its split into pushes.
 *   Map (RR_FRAME_SYMBOLS): d_out is f32 and out = bit ? hi : lo; without the flag d_out is u8 and lo / hi are ignored.
 * NULL + rr_last_error: "unknown hdlc framer flags", said before any device is touched. */
enum { RR_FRAME_FCS = 1, RR_FRAME_G3RUH = 2, RR_FRAME_NRZI = 4, RR_FRAME_SYMBOLS = 8 };
typedef struct {
    size_t start, len;      /* the frame is d_out[start .. start + len) */
    unsigned stuffed;       /* stuffed bits of the frame: len = 320 + 8 L + stuffed, L = the packet's bytes (+ 2 with the FCS) */
    unsigned short fcs;     /* the FCS FcsAdder appended; 0 without RR_FRAME_FCS */
} rr_frame_record;
rr_block *rr_hdlc_framer_create(int flags, float lo, float hi);
/* The elements a push of these packets can produce at most: the sum of 320 + 8 L + floor(8 L / 5), L = lens[p] (+ 2 with the
 * FCS); an all-ones payload reaches it.  (size_t)-1 where that overflows; 0 for a handle that is no framer. */
size_t rr_hdlc_framer_bound(const rr_block *b, const size_t *lens, size_t npackets);
/* Packet p is d_bytes[starts[p] .. starts[p] + lens[p]) of the device buffer d_bytes (n_bytes u8); starts and lens are HOST
 * arrays in the convention of rr_wpcr_process_dev, read before the call returns.  The ranges must lie inside n_bytes ("packet
 * outside the buffer") but may overlap or repeat: the input is only read.  d_out (device, out_cap elements, u8 or f32 by
 * RR_FRAME_SYMBOLS) must hold rr_hdlc_framer_bound elements, else RR_ERR ("output shorter than the framed bits can be"); a bound
 * above 2^30 elements is RR_ERR too.  Every refusal is made before any device is touched and launches nothing.  Elements of
 * d_out at and beyond the produced ones are never written.  Enqueued on hip_stream (used as given) and returns without
 * waiting: 3 launches for the framer, 2 more with RR_FRAME_FCS, 3 more with RR_FRAME_G3RUH or RR_FRAME_NRZI and 1 more with
 * RR_FRAME_SYMBOLS alone — whatever the packets hold.  npackets == 0 launches nothing and leaves the state alone. */
int rr_hdlc_framer_push_dev(rr_block *b, const void *d_bytes, size_t n_bytes, size_t *starts, size_t *lens, size_t npackets,
                            void *d_out, size_t out_cap, void *hip_stream);
/* The same with host pointers: copies the bytes down, runs, waits and copies the *produced elements of the push back. */
int rr_hdlc_framer_push(rr_block *b, const unsigned char *bytes, size_t n_bytes, size_t *starts, size_t *lens, size_t npackets,
                        void *out, size_t out_cap, size_t *produced);
/* One record per packet of the most recent push, in packet order, and the elements it produced.  Waits for that push, writes the
 * first min(*total, cap) records; rec == NULL with cap == 0 only counts (the contract of rr_wpcr_results).  The host buffers
 * behind it are sized from the packet count, and what the device counted is checked against the bound before it is used. */
int rr_hdlc_framer_records(rr_block *b, rr_frame_record *rec, size_t cap, size_t *total, size_t *produced);
/* *tile_bits = the payload bits of one tile of the stuffing scan, which is also the tile of the line coder (tests aim at the
 * seams with it). */
int rr_hdlc_framer_dims(const rr_block *b, size_t *tile_bits);
/* The elements the most recent push of at least one packet produced, where the next device stage can read them: ONE unsigned long
 * long on the device, the word rr_hdlc_framer_records downloads, ordered behind that push on its stream and valid until the next
 * push (the counterpart of rr_symbol_sync_counts_dev).  As the d_counts of rr_fsk_tx_multi_push_dev it takes the host read out of
 * framer -> modulator; for N framers, gather their words with 8-byte device-to-device copies on the same stream.  A push of no
 * packets leaves the word as it was.  NULL for a handle that is no framer. */
const void *rr_hdlc_framer_produced_dev(rr_block *b);

/* HdlcDeframer::new(src, min_size, max_size) (src/hdlc_deframer.rs:80-101) with set_keep_checksum (:119-121) and set_fix_bits
 * (:114-116) as flags: line bits in, checked frames out, the last block of the packet receivers (examples/ax25-9600-rx.rs,
 * ax25-1200-rx.rs, bell202.rs, g3ruh.rs).  A batch block like rr_stream_to_pdu: rr_block_work on the handle is an error.  A push
 * takes the next n bits of the stream, one per u8 (its lowest bit: what rr_bit_decoder writes), and finds the frames whose closing
 * flag ends inside them, bit-identical to the reference's machine (update_state, :123-232) whatever the split into pushes:
 *   the flag needs 8 bits of the stream (Unsynced(0xff) at the start and after every reset, :130-138, 145, 169, 173);
 *   more than 8 max_size collected bits reset the machine before the next bit is looked at (:144-146), so a frame of exactly
 *     max_size bytes is dropped; seven ones reset it (:167-170); two flags sharing their 0 collect fewer than 7 bits and reset it
 *     at the second flag's end (:171-174);
 *   a frame is the destuffed bits without the closing flag's first 7, LSB first, if they are a whole number of at least min_size
 *     bytes (:176-191); with RR_HDLC_KEEP_CHECKSUM every such frame is delivered as it is (:194-197);
 *   without it frames of fewer than 2 bytes vanish (:199-202), the last 2 bytes are the CRC-16/X.25 (calc_crc, :309-315) of the
 *     rest and are stripped; a wrong one counts in crc_error (:214-218) unless RR_HDLC_FIX_BITS repairs it: find_right_crc
 *     (:41-71) flips one data bit, lowest byte and bit first, and delivers the repaired frame (flags bit 0, bitfixed); a single
 *     wrong bit in the CRC field itself counts in bitfixed AND crc_error and delivers nothing.
 * The state between pushes — the machine at the last flag end, the raw bits of the gap still open (at most carry_bits of
 * rr_hdlc_deframer_dims) and the three counters — stays on the device; the host never reads it to decide a size.  The reference's
 * output_space back-pressure (:237-253) has no counterpart: a push delivers every frame of its bits.
 * NULL + rr_last_error, said before any device is touched: "unknown hdlc deframer flags", "hdlc deframer: max_size beyond 65535".
 * min_size 0 and max_size 0 are legal, as in the reference. */
enum { RR_HDLC_KEEP_CHECKSUM = 1, RR_HDLC_FIX_BITS = 2 };       /* set_keep_checksum / set_fix_bits */
typedef struct {
    unsigned long long pos;    /* the "packet_pos" tag (:193): stream position of the closing flag's last bit */
    unsigned long long start;  /* first byte of the frame in the byte arena of this push */
    unsigned len;              /* bytes delivered (FCS stripped unless RR_HDLC_KEEP_CHECKSUM) */
    unsigned flags;            /* bit 0: a data bit was repaired */
} rr_hdlc_frame;               /* 24 bytes */
rr_block *rr_hdlc_deframer_create(size_t min_size, size_t max_size, int flags);
/* The next n bits of the stream from the device buffer d_bits.  RR_ERR before any device is touched: "hdlc deframer: more than
 * 2^30 bits in one push", "hdlc deframer: null bits" (n > 0 with a null buffer).  Enqueued on hip_stream (used as given) and
 * returns without waiting; seven launches whose grids depend on n and max_size alone, never on what the bits hold.  n == 0
 * launches nothing, has no frames and leaves every state alone. */
int rr_hdlc_deframer_push_dev(rr_block *b, const void *d_bits, size_t n, void *hip_stream);
/* The same with a host pointer: copies the bits down, runs and waits. */
int rr_hdlc_deframer_push(rr_block *b, const unsigned char *bits, size_t n);
/* The frames that ended inside the most recent push, ascending by pos.  Waits for that push, writes the first min(*total, cap)
 * records; rec == NULL with cap == 0 only counts (the contract of rr_wpcr_results).  Everything the device wrote is checked
 * against the bounds of the push before it is used ("hdlc deframer: ..." and no frames otherwise). */
int rr_hdlc_frames(rr_block *b, rr_hdlc_frame *rec, size_t cap, size_t *total);
/* The byte arena of the most recent push, which rec.start indexes: *total bytes, the first min(*total, cap) copied.  Bytes that
 * belong to no frame are 0. */
int rr_hdlc_frame_bytes(rr_block *b, unsigned char *out, size_t cap, size_t *total);
/* The same arena on the device for a consumer there (ordered behind the push on its stream); valid until the next push.
 * NULL and *n_total = 0 when the most recent push was empty. */
const void *rr_hdlc_bytes_dev(rr_block *b, size_t *n_total);
/* decoded, crc_error, bitfixed (:92-96) of the handle so far.  Waits for the most recent push. */
int rr_hdlc_stats(rr_block *b, unsigned long long *decoded, unsigned long long *crc_error, unsigned long long *bitfixed);
/* *tile_bits = the bits of one tile of the marking kernels (the first tile of a push begins *carried* bits in front of the push's
 * first bit, so tests aim at the seams through a push of a handle that carries the 8 bits of a fresh stream); *carry_bits = the
 * most bits a handle carries from push to push: M + floor((M - 1) / 5) + 16, M = 8 max_size + 1. */
int rr_hdlc_deframer_dims(const rr_block *b, size_t *tile_bits, size_t *carry_bits);

/* SymbolSync::new(src, sps, max_deviation, TedZeroCrossing, IirFilter::new(taps)) x nstreams (src/symbol_sync.rs:71-98, work
 * :115-217; src/iir_filter.rs:104-125): the symbol clock of the streaming data receivers (examples/ax25-9600-rx.rs:186-193,
 * ax25-1200-rx.rs:293-300, il2p-1200-rx.rs:110-117), between the FM front end (rr_fm_chain / rr_fm_multi / rr_channelizer) and
 * rr_bit_decoder, with the samples, the symbols and the clock state staying on the device.  A batch block like rr_hdlc_deframer:
 * rr_block_work on the handle is an error.  One handle runs nstreams independent SymbolSyncs, each with its own state.
 * EXACT: symbols, clock values and counts are bit-identical to the reference block's, whatever the split of a stream into pushes
 * (its state is per sample; every f32 operation is rounded on its own, in its order).  fill(sps) puts ntaps - 1 copies of sps
 * into a history of deviations, so with the examples' taps the clock starts pinned at sps + max_deviation: reproduced, not repaired.
 * There is no parallel form within one stream: a push is three launches whatever nstreams and the samples are (signs packed 64 to
 * a word; one lane per stream walking them with the reference's loop; a gather), and ONE stream runs on ONE lane, slower than one
 * host core (README, profiles/symsync_probe.md).
 * DEVIATIONS, both refusals: the reference takes any max_deviation and loops forever once clock <= 0, and has no cap on the taps.
 * NULL + rr_last_error, said before any device is touched: "sps must be above 1" (:78; NaN too), "max_deviation out of range"
 * (unless 0 <= max_deviation <= sps / 2), "SymbolSync needs 1 to 8 finite taps", "nstreams out of range" (0 or above 4096).
 * NOT TESTED: after a non-finite clock (overflowing taps only) the block emits nothing more, as the reference would; stream_pos
 * saturates at 2^24 through a run that long without a sign change, as the reference's does.
 * The reference's assert at :157 (stream_pos > last_sym_boundary_pos) cannot fire: the boundary is a copy of an earlier stream_pos,
 *   stream_pos has grown by 1.0 at least once since (below 2^24 + 1 that is never rounded away) and a step back moves both alike.
 * The one at :175 (t > 0) cannot fire: it stands behind t > 0.8 (sps - max_deviation) >= 0.4 sps > 0. */
rr_block *rr_symbol_sync_create(float sps, float max_deviation, const float *taps, size_t ntaps, size_t nstreams);
/* stream c: n samples at d_in + c*in_stride; its symbols at d_syms + c*out_stride, its clock values (d_clock may be NULL:
 * out_clock() never called) at d_clock + c*out_stride.  in_stride >= n, out_stride >= n (a sample emits at most one symbol), the
 * layout of rr_fm_multi_create's output windows.  Elements at and beyond a stream's count are never written.  RR_ERR before any
 * device is touched: a stride below n, n >= 2^31, a null buffer with n > 0.  n == 0 launches nothing, produces 0 for every stream
 * and leaves every state alone.  Asynchronous on hip_stream. */
int rr_symbol_sync_push_dev(rr_block *b, const void *d_in, size_t in_stride, size_t n,
                            void *d_syms, void *d_clock, size_t out_stride, void *hip_stream);
/* The same with host pointers: copies the samples down, runs, waits and copies each stream's produced[c] symbols (and clock values)
 * back. */
int rr_symbol_sync_push(rr_block *b, const float *in, size_t in_stride, size_t n,
                        float *syms, float *clock, size_t out_stride, size_t *produced /* [nstreams] */);
/* symbols of each stream in the most recent push; waits for it (one download of 8*nstreams bytes).  *total = nstreams, the first
 * min(*total, cap) written (the contract of rr_wpcr_results); a count is clamped to the push's n before anybody sees it. */
int rr_symbol_sync_produced(rr_block *b, size_t *produced, size_t cap, size_t *total);
/* the same counts where the next device stage can read them: unsigned long long[nstreams], valid until the next push */
const void *rr_symbol_sync_counts_dev(rr_block *b);
/* *streams_per_wave = 1 (one active lane per wave) or 64: how the clock kernel maps streams to lanes (rr_build_opts.sync_lanes) */
int rr_symbol_sync_dims(const rr_block *b, size_t *streams_per_wave);
/* carried state of one stream after the most recent push (waits): clock, stream_pos, last_sym_boundary_pos, next_sym_middle,
 * last_sign, and the filter history oldest first (*nhist = ntaps - 1, the first min(*nhist, cap) written) */
int rr_debug_symbol_sync_state(rr_block *b, size_t stream, float *four, int *last_sign, float *hist, size_t cap, size_t *nhist);

/* BinarySlicer (src/binary_slicer.rs:17-19) -> [XorConst(1)] -> [NrziDecode (src/nrzi.rs:36-41)] -> [Descrambler::new(mask, seed,
 * len) (src/descrambler.rs:34-39)] -> HdlcDeframer::new(min_size, max_size) (src/hdlc_deframer.rs:80-232) x nstreams, as wired in
 * examples/ax25-9600-rx.rs:195-215: the consumer of rr_symbol_sync.  One handle takes the ragged symbol windows of nstreams
 * streams, with their counts read on the device, and delivers the checked frames of all of them in seven launches whatever
 * nstreams and the symbols are; each stream's decoder and deframer state, its own stream position included, stays on the device.
 * rr_fm_multi -> rr_symbol_sync -> rr_hdlc_receiver is the multi-channel packet receiver with no host round trip before the frames.
 * A batch block like rr_hdlc_deframer: rr_block_work on the handle is an error.
 * EXACT: for every stream, frames, bytes, pos, the repaired flag and the three counters are those of rr_bit_decoder_create(bit_flags,
 * mask, seed, len, 0, 0, 0) on f32 feeding rr_hdlc_deframer_create(min_size, max_size, hdlc_flags) on that stream alone, whatever
 * the split into pushes and whatever the other streams hold.  pos counts that stream's own symbols.  The symbols are sliced and
 * run through the bit chain as 64-bit words inside the deframer's first kernel: no stream of one byte per bit exists.
 * NULL + rr_last_error, said before any device is touched: "nstreams out of range" (0 or above 4096), then the refusals of
 * rr_bit_decoder_create ("unknown bit decoder flags", "descrambler length out of range", "seed wider than the register") and of
 * rr_hdlc_deframer_create ("unknown hdlc deframer flags", "hdlc deframer: max_size beyond 65535").
 * Device memory: 2 * nstreams * carry_bits bytes of carried bits (rr_hdlc_receiver_dims) live as long as the handle.
 * NOT TESTED: max_size above a few hundred with many streams; a push of 2^30 symbols. */
typedef struct {
    unsigned long long pos;    /* stream position (in that stream's own symbols) of the closing flag's last bit */
    unsigned long long start;  /* first byte of the frame in the byte arena of this push (absolute: every stream owns a region) */
    unsigned len;              /* bytes delivered (FCS stripped unless RR_HDLC_KEEP_CHECKSUM) */
    unsigned flags;            /* bit 0: a data bit was repaired */
    unsigned stream;
    unsigned reserved;         /* 0 */
} rr_hdlc_stream_frame;        /* 32 bytes */
rr_block *rr_hdlc_receiver_create(size_t nstreams, int bit_flags /* RR_BITS_* */, unsigned long long mask, unsigned long long seed,
                                  unsigned len, size_t min_size, size_t max_size, int hdlc_flags /* RR_HDLC_* */);
/* stream c: the next min(d_counts[c], n_cap) f32 symbols at d_syms + c*stride, the layout rr_symbol_sync_push_dev writes.
 * d_counts: unsigned long long[nstreams] on the device, the pointer rr_symbol_sync_counts_dev returns, read there and clamped to
 * n_cap before it is used; NULL: every stream has n_cap.  Elements at and beyond a stream's count are never read.  A stream whose
 * count is 0 keeps every piece of its state.  RR_ERR before any device is touched: "hdlc receiver: stride shorter than n_cap",
 * "hdlc receiver: more than 2^30 symbols in one push" (nstreams * n_cap), "hdlc receiver: null symbols" (n_cap > 0 with a null
 * buffer).  n_cap == 0 launches nothing, has no frames and leaves every state alone.  Asynchronous on hip_stream (used as given). */
int rr_hdlc_receiver_push_dev(rr_block *b, const void *d_syms, size_t stride, size_t n_cap, const void *d_counts, void *hip_stream);
/* The same with host pointers (counts may be NULL): copies symbols and counts down, runs and waits. */
int rr_hdlc_receiver_push(rr_block *b, const float *syms, size_t stride, size_t n_cap, const size_t *counts /* [nstreams] or NULL */);
/* The frames of all streams that ended inside the most recent push, ascending by (stream, pos).  Waits for that push, writes the
 * first min(*total, cap) records; rec == NULL with cap == 0 only counts (the contract of rr_wpcr_results).  Everything the device
 * wrote — the record count, every record's stream, length, place in its stream's region of the arena, position and flags, the
 * streams' positions and counters — is checked against the host's own bounds before it is used ("hdlc receiver: ..." and no frames
 * otherwise). */
int rr_hdlc_receiver_frames(rr_block *b, rr_hdlc_stream_frame *rec, size_t cap, size_t *total);
/* The byte arena of the most recent push, which rec.start indexes: *total bytes (nstreams equal regions), the first
 * min(*total, cap) copied.  Bytes that belong to no frame are 0. */
int rr_hdlc_receiver_frame_bytes(rr_block *b, unsigned char *out, size_t cap, size_t *total);
/* The same arena on the device (ordered behind the push on its stream); valid until the next push.  NULL and *n_total = 0 when
 * the most recent push was empty. */
const void *rr_hdlc_receiver_bytes_dev(rr_block *b, size_t *n_total);
/* decoded, crc_error, bitfixed of every stream so far; waits for the most recent push.  *total = nstreams, the first
 * min(*total, cap) of each array written (the contract of rr_symbol_sync_produced); an array may be NULL. */
int rr_hdlc_receiver_stats(rr_block *b, unsigned long long *decoded, unsigned long long *crc_error, unsigned long long *bitfixed,
                           size_t cap, size_t *total);
/* symbols every stream has taken so far (its stream position); waits for the most recent push.  Same contract. */
int rr_hdlc_receiver_consumed(rr_block *b, unsigned long long *symbols, size_t cap, size_t *total);
/* *tile_bits, *carry_bits: as rr_hdlc_deframer_dims, for every stream. */
int rr_hdlc_receiver_dims(const rr_block *b, size_t *tile_bits, size_t *carry_bits);

/* BinarySlicer (src/binary_slicer.rs:17-19) -> [XorConst(1)] -> CorrelateAccessCodeTag::new(il2p_deframer::SYNC_WORD, "sync",
 * allowed_diffs) (src/correlate_access_code.rs:93-118) -> Il2pDeframer (src/il2p_deframer.rs:172-237, 247-319) x nstreams, as
 * wired in examples/il2p-1200-rx.rs:118-137: the consumer of rr_symbol_sync for IL2P.  One handle takes the ragged symbol windows
 * of nstreams streams, with their counts read on the device, and delivers the parsed headers of all of them in three launches
 * whatever nstreams and the symbols are; each stream's state (its position, the bits-seen count, how far the open header still
 * blocks, its last 192 sliced bits as three words) stays on the device.  rr_fm_multi -> rr_afsk_demod -> rr_symbol_sync ->
 * rr_il2p_receiver is the whole graph of il2p-1200-rx for N channels, with no host round trip before the headers.
 * A batch block like rr_hdlc_receiver: rr_block_work on the handle is an error.
 * EXACT, per stream and whatever the split into pushes and the other streams hold: b[i] = (x[i] > 0.0f) ^ invert (NaN, +-0.0 and
 * -Inf slice to 0 before the inversion); position i carries a tag when 24 bits of the stream have been seen and b[i-23 ..= i]
 * differs from SYNC_WORD (0xF15E48, oldest bit first) in at most allowed_diffs places; the first tag at p >= free_from (0 at the
 * start) is accepted, its header is the 120 bits b[p+1 .. p+121), then free_from = p + 121; every other tag is dropped.  The
 * header is descrambled (Lfsr::new(0x108, 0x1f0), :101-128, 257), packed MSB first into 15 bytes (:130-141) and its first 13 bytes
 * parsed as Header::parse (:289-319) with decode_callsign (:265-274).  The reference strips the 2 parity bytes unchecked (TODO at
 * :209) and delivers no payload (TODO at :186); so does this block, and it keeps the parity bytes in raw.
 * NULL + rr_last_error, said before any device is touched: "nstreams out of range" (0 or above 4096), "il2p receiver: unknown bit
 * flags" (anything other than 0 or RR_BITS_INVERT).  allowed_diffs takes any value; 24 and above: every position from 23 on matches.
 * Device memory: 2 * 64 bytes of state per stream live as long as the handle (rr_il2p_receiver_dims: carry_bits = 192).
 * NOT TESTED: a push of 2^30 symbols; more than 4096 tiles in one stream on the device. */
typedef struct {
    unsigned long long pos;      /* stream position (that stream's own symbols) of the sync tag: the sync word's last bit */
    unsigned stream;
    unsigned short payload_size; /* 10 bits */
    unsigned char pid;           /* 4 bits */
    unsigned char control;       /* 7 bits */
    unsigned char flags;         /* bit 0 ui, bit 1 fec, bit 2 hdrtype1 */
    unsigned char diffs;         /* the tag's value */
    unsigned char dst_ssid, src_ssid;
    unsigned char raw[15];       /* the descrambled header, its 2 parity bytes last (kept: a host may run the RS check) */
    char dst[7], src[7];         /* decode_callsign, NUL padded */
    unsigned char reserved[15];  /* 0 */
} rr_il2p_header;                /* 64 bytes */
#if defined(__cplusplus)
static_assert(sizeof(rr_il2p_header) == 64, "rr_il2p_header is 64 bytes");
#else
_Static_assert(sizeof(rr_il2p_header) == 64, "rr_il2p_header is 64 bytes");
#endif
rr_block *rr_il2p_receiver_create(size_t nstreams, int bit_flags /* RR_BITS_INVERT or 0 */, size_t allowed_diffs);
/* stream c: the next min(d_counts[c], n_cap) f32 symbols at d_syms + c*stride, the layout rr_symbol_sync_push_dev writes.
 * d_counts: unsigned long long[nstreams] on the device, the pointer rr_symbol_sync_counts_dev returns, read there and clamped to
 * n_cap before it is used; NULL: every stream has n_cap.  Elements at and beyond a stream's count are never read.  A stream whose
 * count is 0 keeps every piece of its state.  RR_ERR before any device is touched: "il2p receiver: stride shorter than n_cap",
 * "il2p receiver: more than 2^30 symbols in one push" (nstreams * n_cap), "il2p receiver: null symbols" (n_cap > 0 with a null
 * buffer).  n_cap == 0 launches nothing, has no headers and leaves every state alone.  Asynchronous on hip_stream (used as given). */
int rr_il2p_receiver_push_dev(rr_block *b, const void *d_syms, size_t stride, size_t n_cap, const void *d_counts, void *hip_stream);
/* The same with host pointers (counts may be NULL): copies symbols and counts down, runs and waits. */
int rr_il2p_receiver_push(rr_block *b, const float *syms, size_t stride, size_t n_cap, const size_t *counts /* [nstreams] or NULL */);
/* The headers of all streams whose 120th bit lay inside the most recent push (il2p_deframer.rs:206-213), ascending by (stream,
 * pos).  Waits for that push, writes the first min(*total, cap) records; rec == NULL with cap == 0 only counts (the contract of
 * rr_wpcr_results).  The list holds floor((n_cap + 119) / 121) + 1 records per stream, more than a push can emit, so no record is
 * ever dropped.  Everything the device wrote — the record count, every record's stream, its position inside that stream's range of
 * the push, positions of one stream at least 121 apart, the fields' ranges — is checked against the host's own bounds before it is
 * used ("il2p receiver: ..." and no headers otherwise). */
int rr_il2p_receiver_headers(rr_block *b, rr_il2p_header *rec, size_t cap, size_t *total);
/* headers delivered and sync tags seen (accepted or not, correlate_access_code.rs:110-116) of every stream since creation; waits
 * for the most recent push.  *total = nstreams, the first min(*total, cap) of each array written (the contract of
 * rr_symbol_sync_produced); an array may be NULL. */
int rr_il2p_receiver_stats(rr_block *b, unsigned long long *headers, unsigned long long *syncs, size_t cap, size_t *total);
/* symbols every stream has taken so far (its stream position); waits for the most recent push.  Same contract. */
int rr_il2p_receiver_consumed(rr_block *b, unsigned long long *symbols, size_t cap, size_t *total);
/* *tile_bits: symbols of one tile of the kernels; *carry_bits: sliced bits every stream keeps between pushes (23 for the
 * correlator, 120 for an open header's tag and bits, rounded up to words) */
int rr_il2p_receiver_dims(const rr_block *b, size_t *tile_bits, size_t *carry_bits);

/* [ComplexToMag2 ->] PwmDecoder::builder(high_threshold, short_width, long_width, frame_gap, reset_gap) with every builder
 * setting (src/pwm_decoder.rs:165-266; process :385-513): OOK power samples in, PWM frames out, the whole graph of
 * examples/restaurant_pager.rs behind one handle.  A batch block like rr_hdlc_deframer: rr_block_work on the handle is an error.
 * A push takes the next n samples of the stream and delivers the frames of every transmission whose reset sample lies inside it,
 * bit-identical to the reference's machine whatever the split into pushes (comparisons and integer counts only):
 *   the slicer (:386-424) starts low; in low p <= high_threshold stays low, in high p >= low_threshold stays high, so a NaN rises
 *     from low and falls from high; the first sample of a run belongs to it;
 *   a pulse is short or long when its width lies within pulse_tolerance of that nominal width, the nearer one when both do, short
 *     on a tie (:434-446); it is data when the low run behind it is shorter than frame_gap, and, without RR_PWM_GAP_DELIMITER,
 *     also when it is the last one in front of a frame gap (:399-402, :412-416); its bit is (short == short_is_one);
 *   the gap events fire on the sample at which the low run EQUALS frame_gap / reset_gap (:398-409), the frame first;
 *   a frame is accepted when every data pulse is valid, it has 1 .. max_frame_bits of them (one more rejects it up to its gap,
 *     :447-460) and exactly frame_bits if that is not 0 (:471-481); first_sample is the rise of its first pulse;
 *   within a transmission the first max_distinct_frames distinct patterns are the candidates, `repeats` counts the accepted
 *     frames equal to each (:485-497); the reset event delivers those with repeats >= min_repeats in candidate order (:502-513).
 * in_elem_size 4: the f32 power stream.  8: Complex samples, norm_sqr with the reference's three f32 roundings in front, so both
 * see the same power bit for bit.  Both thresholds and the tolerance are explicit (the builder's defaults, high / 2 and
 * |long - short| / 2, are the mirrors' business); frame_bits 0 is None.
 * The state between pushes — the slicer state, the open run's length (64 bits), the pending pulse, the open frame (bits, count,
 * invalid flag, start), the candidate table and the stream position — stays on the device and is bounded by the settings; the
 * host never reads it to decide a size.  The reference's pending-queue back-pressure (:602-610) has no counterpart.
 * NULL + rr_last_error, said before any device is touched: every refusal of validate() (:101-162) in its words ("PwmDecoder high
 * threshold must be finite and greater than zero", ...), "unknown pwm decoder flags", "pwm decoder: Float (4) or Complex (8)
 * input only", and the limits of a handle, refused, never clamped: "pwm decoder: max_frame_bits beyond 16384", "pwm decoder:
 * max_distinct_frames beyond 1024", "pwm decoder: max_frame_bits x max_distinct_frames beyond 4194304" (the defaults, 4096 x 256,
 * are a quarter of that), "pwm decoder: width or gap beyond 2^62", "pwm decoder: min_repeats beyond 2^32 - 1". */
enum { RR_PWM_SHORT_IS_ZERO = 1, RR_PWM_GAP_DELIMITER = 2 };    /* short_is_one(false) / gap_pulse(PwmGapPulse::Delimiter) */
typedef struct {
    unsigned long long first_sample;   /* PwmFrame::first_sample: stream position of the first copy's first rise */
    unsigned long long start;          /* first bit of the frame in the bit arena of this push */
    unsigned len;                      /* PwmFrame::len: bits */
    unsigned repeats;                  /* PwmFrame::repeats */
} rr_pwm_frame;                        /* 24 bytes */
rr_block *rr_pwm_decoder_create(float high_threshold, float low_threshold, size_t short_width, size_t long_width,
                                size_t pulse_tolerance, size_t frame_gap, size_t reset_gap, size_t frame_bits, size_t max_frame_bits,
                                size_t max_distinct_frames, size_t min_repeats, int flags, size_t in_elem_size);
/* The next n samples of the stream from the device buffer d_samples.  RR_ERR before any device is touched: "pwm decoder: more
 * than 2^30 samples in one push", "pwm decoder: null samples" (n > 0 with a null buffer), "pwm decoder: push after flush".
 * Enqueued on hip_stream (used as given) and returns without waiting; SEVEN launches whose grids depend on n and the settings
 * alone, never on what the samples hold (silence, one burst or an edge on every sample).  Everything is sized from n and the
 * settings: n edges, n / 2 + 2 pulses, max_distinct_frames + n / 2 + 2 records.  n == 0 launches nothing, has no frames and
 * leaves every state alone. */
int rr_pwm_decoder_push_dev(rr_block *b, const void *d_samples, size_t n, void *hip_stream);
/* The same with a host pointer: copies the samples down, runs and waits. */
int rr_pwm_decoder_push(rr_block *b, const void *samples, size_t n);
/* EOF (finalize_eof, :612-618): delivers the open transmission's candidates as a push of its own (two launches) and throws the
 * open frame away.  Afterwards the handle refuses pushes and flushes ("pwm decoder: push after flush"). */
int rr_pwm_decoder_flush(rr_block *b, void *hip_stream);
/* The frames the most recent push or flush delivered, in the reference's delivery order.  Waits for it, writes the first
 * min(*total, cap) records; rec == NULL with cap == 0 only counts (the contract of rr_hdlc_frames).  Everything the device wrote
 * is checked against the bounds of the push before it is used ("pwm decoder: ..." and no frames otherwise). */
int rr_pwm_frames(rr_block *b, rr_pwm_frame *rec, size_t cap, size_t *total);
/* The bit arena of the most recent push or flush, which rec.start indexes: one u8 of 0 or 1 per bit (PwmFrame::bits, and what the
 * bit blocks here take), frame behind frame.  *total bits, the first min(*total, cap) copied. */
int rr_pwm_frame_bits(rr_block *b, unsigned char *out, size_t cap, size_t *total);
/* The same arena on the device (ordered behind the push on its stream); valid until the next push.  Waits for the push (the
 * arena's length is the device's own, checked count).  NULL and *n_total = 0 when nothing was delivered. */
const void *rr_pwm_bits_dev(rr_block *b, size_t *n_total);
/* *tile_samples = the samples of one tile of the slicer kernels; tile t of a push begins at its sample t * tile_samples.  The two
 * one-workgroup scans take 1024 tiles in one go. */
int rr_pwm_decoder_dims(const rr_block *b, size_t *tile_samples);

/* The tone demodulator of the 1200-baud AFSK receivers (examples/ax25-1200-rx.rs:238-247, il2p-1200-rx.rs:81-89),
 *   Hilbert::new(_, hilbert_ntaps, window) -> QuadratureDemod::new(_, gain) -> FftFilterFloat::new(_, taps) -> AddConst::new(_, offset)
 * x nstreams behind one handle, between the audio of rr_fm_multi / rr_fm_receiver and rr_symbol_sync, with the samples and every
 * stream's state staying on the device.  A batch block like rr_symbol_sync: rr_block_work on the handle is an error.
 * DEFINITION, per stream (x = every sample pushed so far, H = hilbert_ntaps, L = ntaps, hil = hilbert_taps(make_window(window, H, parm))):
 *   xp     = H zeros ++ x
 *   a[m]   = (xp[m + H/2], sum_j hil[H-1-j] xp[m + j])        j = 0 .. H-1
 *   d[m]   = gain * atan2(Im, Re) of a[m+1] conj(a[m])        d[<0] = 0
 *   out[i] = (sum_j taps[j] d[i - j]) + offset                one f32 add, last
 * After T samples in all a stream has delivered exactly max(T - 1, 0) outputs, the reference's whole-stream count.  The bits of
 * out do not depend on how the stream was cut into pushes, on where a tile starts or on what the other streams hold: every output
 * is one fixed sequence of f32 operations (afsk_core.hpp), and stream c of an N-stream handle equals a 1-stream handle fed row c.
 * Against the float64 form of the definition the error is within sum_j |taps[j]| b[i-j] + 1e-5 max|y|, b the bound of an angle
 * whose two samples are 1e-5 max|a| off (tests/afsk_model.py).
 * ONE launch per push whatever nstreams and n are: the low-pass is a direct sum (L multiply-adds per output), not the reference's
 * overlap-save transform.  A handle carries the latest L + H samples of every stream on the device (rr_afsk_demod_dims).
 * DEVIATIONS: the reference's FftFilterFloat withholds a partial block and never flushes it; this delivers every output whose
 * inputs exist (same values, a later tail).  A NaN at x[k] makes exactly outputs k .. k + H + L - 1 NaN and touches no other bit
 * (the reference poisons whole transform blocks, a superset); after +-Inf the set is not pinned.
 * NULL + rr_last_error, said before any device is touched: "nstreams out of range" (0 or above 4096), "hilbert filter len must be
 * odd and greater than 1" (hilbert.rs:48), "hilbert filter len above 1023", "unknown window, or a non-finite window parameter",
 * "AfskDemod needs 1 to 4096 finite taps" (refused beyond, never clamped), "gain and offset must be finite". */
rr_block *rr_afsk_demod_create(size_t nstreams, size_t hilbert_ntaps, int window, float window_parm, float gain,
                               const float *taps, size_t ntaps, float offset);
/* stream c: its next n samples at d_in + c*in_stride, its *produced outputs at d_out + c*out_stride (f32 elements): the layout
 * rr_fm_multi_create writes and rr_symbol_sync_push_dev reads.  *produced (may be NULL) depends on lengths only, is the same for
 * every stream and is written before the call returns: n, or n - 1 for the push that starts the streams; it is the n of the
 * following rr_symbol_sync_push_dev.  Nothing at or beyond a stream's count is written.  RR_ERR before any device is touched: a
 * stride below n, nstreams * n above 2^30, a null buffer with n > 0.  n == 0 launches nothing and leaves every state alone.
 * Asynchronous on hip_stream. */
int rr_afsk_demod_push_dev(rr_block *b, const void *d_in, size_t in_stride, size_t n,
                           void *d_out, size_t out_stride, size_t *produced, void *hip_stream);
/* The same with host pointers: copies the samples down, runs, waits and copies each stream's outputs back. */
int rr_afsk_demod_push(rr_block *b, const float *in, size_t in_stride, size_t n, float *out, size_t out_stride, size_t *produced);
/* *tile_samples = outputs of one workgroup (2048), *carry_samples = samples of a stream a handle carries (L + H) */
int rr_afsk_demod_dims(const rr_block *b, size_t *tile_samples, size_t *carry_samples);

/* The audio path of examples/airspy_am_decode.rs behind the RF filter,
 *   Map(|v| v.norm()) -> FftFilterFloat::new(_, taps) -> RationalResampler::new(_, interp, deci) -> MultiplyConst::new(_, scale)
 * x nstreams behind one handle, behind the Complex windows of rr_channelizer_create (or rr_fftfilter), with the samples and every
 * stream's state staying on the device.  A batch block like rr_afsk_demod: rr_block_work on the handle is an error.
 * DEFINITION, per stream (x = every Complex sample pushed so far, L = ntaps, I:D = interp:deci after gcd reduction):
 *   m[k]   = fl32( sqrt( f64(x[k].re)^2 + f64(x[k].im)^2 ) )      m[k < 0] = 0   (FftFilterFloat starts from zero history)
 *   y[i]   = sum_j taps[j] m[i - j]                               j = 0 .. L-1, f32
 *   out[o] = scale * y[ floor(o D / I) ]                          one f32 multiply, last
 * After N samples in all a stream has delivered exactly ceil(N I / D) outputs (src/rational_resampler.rs:183-198).  The squares
 * of f32 values are exact in f64, so m is one f64 add, one correctly rounded f64 sqrt and one narrowing: the bits of glibc's
 * hypotf, which Complex::norm() calls, for every finite input.  The bits of out do not depend on how the stream was cut into
 * pushes, on which tile or lane computed them or on what the other streams hold: every output is one fixed sequence of f32
 * operations that L alone determines (am_core.hpp: 64 strided partial sums of fmaf, a six-level tree of adds, the multiply), and
 * stream c of an N-stream handle equals a 1-stream handle fed row c.
 * BOUND: against the float64 form of the definition (exact m, exact sums) each output is within
 *   B[o] = 1.01 (L + 2) 2^-24 |scale| sum_j |taps[j]| m64[p(o) - j],  p(o) = floor(o D / I)
 * (outputs that are not subnormal).
 * ONE launch per push whatever nstreams, n, L and the ratio are.  The filter is a direct, decimate-first sum: only the y the
 * resampler picks are computed (L multiply-adds per OUTPUT), not the reference's overlap-save transform at the input rate.  A
 * handle carries the latest L - 1 magnitudes of every stream on the device (rr_am_demod_dims); the counts live on the host.
 * DEVIATIONS: the reference's FftFilterFloat withholds a partial block and never flushes it; this delivers every output whose
 * inputs exist (same values, a later tail).  A NaN at x[k] makes NaN exactly the outputs o with p(o) - L + 1 <= k <= p(o) and
 * touches no other bit (the reference poisons whole transform blocks, a superset); after +-Inf the set is not pinned
 * (hypot(Inf, NaN) is Inf in libm and NaN by the definition).
 * NULL + rr_last_error, said before any device is touched: "nstreams out of range" (0 or above 4096), "AmDemod needs 1 to 16384
 * finite taps" (refused beyond, never clamped), "RationalResampler created using deci 0", "RationalResampler created using
 * interp 0" (the reference's sentences), "am demod: reduced ratio part above 2^31", "scale must be finite". */
rr_block *rr_am_demod_create(size_t nstreams, const float *taps, size_t ntaps, size_t interp, size_t deci, float scale);
/* stream c: its next n samples at d_in + c*in_stride (rr_c32 elements: the out_cap windows rr_channelizer_create writes), its
 * *produced outputs at d_out + c*out_stride (f32 elements).  A push of n samples behind N0 earlier ones writes outputs
 * [O(N0), O(N0 + n)), O(N) = ceil(N I / D).  *produced (may be NULL) depends on lengths only, is the same for every stream and is
 * written before the call returns.  Nothing at or beyond a stream's count is written.  RR_ERR, nothing launched and nothing
 * changed: in_stride below n, out_stride below produced, nstreams * n or nstreams * produced above 2^30, a null buffer with work
 * to do.  n == 0 launches nothing and leaves every state alone.  Asynchronous on hip_stream. */
int rr_am_demod_push_dev(rr_block *b, const void *d_in, size_t in_stride, size_t n,
                         void *d_out, size_t out_stride, size_t *produced, void *hip_stream);
/* The same with host pointers: copies the samples down, runs, waits and copies each stream's outputs back. */
int rr_am_demod_push(rr_block *b, const rr_c32 *in, size_t in_stride, size_t n, float *out, size_t out_stride, size_t *produced);
/* *tile_outputs = outputs of one workgroup (32 .. 192, chosen at create from (I, D, L)), *carry_samples = magnitudes of a stream
 * a handle carries (L - 1) */
int rr_am_demod_dims(const rr_block *b, size_t *tile_outputs, size_t *carry_samples);

/* The modulators of the reference's two packet transmitters, line bits in, baseband out, in PDU form (rr_block_work on the handle
 * is an error).  Bits are u8 as rr_hdlc_framer_push_dev writes them without RR_FRAME_SYMBOLS; a byte is 1 when it is nonzero (the
 * reference's `s > 0`).  Both ratios are gcd-reduced; a RationalResampler is out[m] = in[floor(m D / I)] and has made ceil(N I / D)
 * outputs after N inputs (src/rational_resampler.rs:183-198).
 *   RR_FSK_TX_AFSK    examples/bell202.rs:166-183 behind its NrziEncode: RationalResampler(interp1, deci1) -> Map(bit > 0 ? hi : lo)
 *                     -> Vco(k1) -> Map(.re) -> MultiplyConst(gain) -> RationalResampler(interp2, deci2) -> Vco(k2)
 *                       a[m]   = fl32(fl32(sin p1[m]) * gain), p1 the f64 phase of Vco(k1) over level[m] = bit[floor(m D1 / I1)] ? hi : lo
 *                       out[o] = (sin p2, cos p2), p2 += k2 * a[floor(o D2 / I2)] once per OUTPUT sample (src/vco.rs:9-37)
 *   RR_FSK_TX_DIRECT  examples/g3ruh.rs:256-272 behind its NrziEncode and in front of its FftFilter: RationalResampler -> Map ->
 *                     Vco(k1) -> MultiplyConst(gain) -> RationalResampler
 *                       out[o] = gain * (sin, cos)(p1[floor(o D2 / I2)]); k2_bits is ignored
 * A push of n bits behind N0 earlier ones makes the audio samples [A(N0), A(N0 + n)), A(N) = ceil(N I1 / D1), and the outputs
 * [O(A(N0)), O(A(N0 + n))), O(A) = ceil(A I2 / D2): everything its bits produce, no run split across pushes.  Both phases stay
 * on the device; counts depend on lengths only.  Every scan runs at the audio rate and the output-rate kernel is a map (kernels_tx.hip
 * has the launch counts).  Accuracy, against the exact phase in long double (tests/tx_model.py), sample indices
 * from the stream's start: audio and DIRECT components within |gain| (2^-24 + (m + 1)(2^-48 + d1 2^-52)), d1 = max |k1 level|; AFSK
 * components within 2^-25 + (o + 1)(2^-48 + d2 2^-52), d2 = |k2| max |a|, of the truth computed from the a[] the same push wrote.
 * Different splits into pushes are each within the bound, not bit-identical; the same pushes twice give the same bits.
 * NULL + rr_last_error, said before any device is touched: "fsk tx: unknown mode", "interpolation and decimation must be nonzero"
 * (the reference's Err), "fsk tx: reduced ratio part above 2^31", "fsk tx: lo and hi must be finite", "fsk tx: gain must be
 * finite", "fsk tx: k1 and k2 must be finite". */
enum { RR_FSK_TX_DIRECT = 0, RR_FSK_TX_AFSK = 1 };
rr_block *rr_fsk_tx_create(int mode, size_t interp1, size_t deci1, float lo, float hi, unsigned long long k1_bits, float gain,
                           size_t interp2, size_t deci2, unsigned long long k2_bits);
/* What the NEXT push of n_bits makes (either pointer may be NULL).  RR_ERR where that push would be refused for its length. */
int rr_fsk_tx_count(const rr_block *b, size_t n_bits, size_t *n_audio, size_t *n_out);
/* d_out: *n_out Complex (re = sin, im = cos); d_audio: f32, may be NULL, must be NULL in DIRECT mode, receives the *n_audio
 * samples a[] (the sound-card signal of bell202.rs).  The counts (pointers may be NULL) are written before the call returns;
 * nothing at or beyond them is written.  RR_ERR before any device is touched, each with its own sentence: a d_audio in DIRECT
 * mode, more than 2^30 bits, audio samples or outputs in one push, an output position beyond 2^62, a null buffer on a push that
 * needs it, out_cap or audio_cap below the counts.  n_bits == 0 launches nothing and leaves every state alone.  Asynchronous on
 * hip_stream. */
int rr_fsk_tx_push_dev(rr_block *b, const void *d_bits, size_t n_bits, void *d_out, size_t out_cap, void *d_audio, size_t audio_cap,
                       size_t *n_out, size_t *n_audio, void *hip_stream);
/* The same with host pointers: copies the bits down, runs, waits and copies the produced elements back. */
int rr_fsk_tx_push(rr_block *b, const void *bits, size_t n_bits, rr_c32 *out, size_t out_cap, float *audio, size_t audio_cap,
                   size_t *n_out, size_t *n_audio);
/* *audio_tile = audio samples of one scan tile (2048), *out_tile = outputs of one workgroup of the map kernel (2048),
 * *scan_chunk_tiles = audio tiles one pass of the tile-level scans takes (4096) */
int rr_fsk_tx_dims(const rr_block *b, size_t *audio_tile, size_t *out_tile, size_t *scan_chunk_tiles);

/* rr_fsk_tx for nstreams streams that share one parameter set, behind one handle: the transmit counterpart of rr_afsk_demod ->
 * rr_symbol_sync -> rr_hdlc_receiver.  Every stream's state (where its two resamplers stand, both phases) stays on the device, and
 * the ragged bit counts of a push are read there under the contract of rr_hdlc_receiver_push_dev, so rr_hdlc_framer_push_dev ->
 * rr_fsk_tx_multi_push_dev needs no host read (rr_hdlc_framer_produced_dev).  A batch block: rr_block_work on the handle is an error.
 * Each stream's push is planned on the device from its own carried position and count, and runs the general path of rr_fsk_tx
 * (the kernels' bodies are shared) with tiles that start at the stream's own push start: a stream's out, audio and counts are
 * bit-identical to an rr_fsk_tx handle given the same pushes wherever each of those pushes makes no audio sample or more than
 * one audio tile (rr_fsk_tx_multi_dims), and do not depend on n_cap, the strides, nstreams or the other streams.  A push of 1 ..
 * audio_tile audio samples takes rr_fsk_tx's one-tile path there and the general path here: both inside the bounds of rr_fsk_tx,
 * not bit-identical.  Launches of a push: 6 (AFSK) or 5 (DIRECT) whatever the counts, the bits and nstreams are; 0 for n_cap == 0.
 * NULL + rr_last_error, said before any device is touched: the refusals of rr_fsk_tx_create, then "nstreams out of range" (0 or
 * above 65535, the grid's y as in rr_afsk_demod_create).
 * NOT TESTED: more than 64 streams except in the timing probe; pushes near 2^30 elements; positions near 2^62. */
rr_block *rr_fsk_tx_multi_create(size_t nstreams, int mode, size_t interp1, size_t deci1, float lo, float hi,
                                 unsigned long long k1_bits, float gain, size_t interp2, size_t deci2, unsigned long long k2_bits);
/* The most ONE stream can make from n_cap bits whatever its residues: *audio_cap = ceil(n_cap I1 / D1), *out_cap = ceil(*audio_cap
 * I2 / D2) on the reduced ratios, saturated at the largest size_t (either pointer may be NULL).  What the strides of a push must
 * hold, and what its scratch and grids are sized from (the role rr_hdlc_framer_bound has for the framer). */
int rr_fsk_tx_multi_bound(const rr_block *b, size_t n_cap, size_t *audio_cap, size_t *out_cap);
/* stream c: the next min(d_counts[c], n_cap) u8 bits at d_bits + c*bits_stride; its outputs (Complex) to d_out + c*out_stride; in
 * AFSK mode with d_audio non-NULL its audio (f32) to d_audio + c*audio_stride.  d_counts: unsigned long long[nstreams] on the
 * device, read there and clamped to n_cap before it is used (the contract of rr_hdlc_receiver_push_dev); NULL: every stream has
 * n_cap.  Bits at and beyond a stream's count are never read; outputs and audio at and beyond a stream's own counts are never
 * written.  A stream whose count is 0 keeps every piece of its state; one whose bits make no audio sample moves only its first
 * resampler.  RR_ERR before any device is touched, nothing launched: "fsk tx multi: DIRECT mode has no audio output", "... more than
 * 2^30 bits of a stream in one push" (n_cap), "... more than 2^30 audio samples of all streams in one push" / "... outputs ..."
 * (nstreams times the bound), "... output position beyond 2^62" (judged from the sum of the n_cap of all pushes, an upper bound of
 * every stream's bit position: the host does not know the device's), "... bits_stride below n_cap", "... out_stride below the outputs
 * a stream can make", "... audio_stride below the audio samples a stream can make", "... null bit buffer", "... null output buffer".
 * n_cap == 0 launches nothing, makes nothing and leaves every state alone.  Asynchronous on hip_stream (used as given). */
int rr_fsk_tx_multi_push_dev(rr_block *b, const void *d_bits, size_t bits_stride, size_t n_cap, const void *d_counts,
                             void *d_out, size_t out_stride, void *d_audio, size_t audio_stride, void *hip_stream);
/* The same with host pointers (counts, audio, n_out and n_audio may be NULL): copies the bits the counts cover and the counts
 * down, runs, waits and copies what each stream made back (the shape of rr_symbol_sync_push). */
int rr_fsk_tx_multi_push(rr_block *b, const unsigned char *bits, size_t bits_stride, size_t n_cap, const size_t *counts,
                         rr_c32 *out, size_t out_stride, float *audio, size_t audio_stride,
                         size_t *n_out /* [nstreams] */, size_t *n_audio /* [nstreams] */);
/* What each stream made in the most recent push; waits for it (one download of 16*nstreams bytes).  *total = nstreams, the first
 * min(*total, cap) of each array written, an array may be NULL (the contract of rr_symbol_sync_produced); every value is checked
 * against the bound of the push before anybody sees it ("fsk tx multi: the device's counts exceed the bound of the push"). */
int rr_fsk_tx_multi_counts(rr_block *b, size_t *n_audio, size_t *n_out, size_t cap, size_t *total);
/* the same counts where the next device stage can read them: unsigned long long[2][nstreams], audio counts then output counts,
 * valid until the next push (as rr_symbol_sync_counts_dev) */
const void *rr_fsk_tx_multi_counts_dev(rr_block *b);
/* Each stream's bits taken, audio samples and outputs made so far; waits for the most recent push (the shape of
 * rr_hdlc_receiver_consumed; an array may be NULL).  For the tests: nothing else needs the positions on the host. */
int rr_fsk_tx_multi_positions(rr_block *b, unsigned long long *bits, unsigned long long *audio, unsigned long long *out,
                              size_t cap, size_t *total);
/* as rr_fsk_tx_dims */
int rr_fsk_tx_multi_dims(const rr_block *b, size_t *audio_tile, size_t *out_tile, size_t *scan_chunk_tiles);

/* Graph-level fusion of Hilbert::new(src, hilbert_ntaps, &window) (src/hilbert.rs:38-61) ->
 * FirFilter::<Complex>::builder(taps).deci(deci)[.translate(samp_rate, freq)].build(_) (src/fir.rs:303-386,476-486)
 * as wired in examples/ax25-1200-rx.rs:238-247: f32 in, Complex out, ONE decimating FIR with the composite
 * Complex taps (Hilbert transformer convolved with `taps`, formed in f64).  Whole-stream output equals the
 * two blocks in sequence to f32 rounding; work() follows FirFilter's protocol on the real input
 * (WAIT_SRC(ntaps+deci-1), consumes deci*floor((len-ntaps+1)/deci), RR_AGAIN). */
rr_block *rr_hilbert_fir_create(size_t hilbert_ntaps, int window, float window_parm, const rr_c32 *taps, size_t ntaps,
                                size_t deci, int translate, float samp_rate, float freq);

/* `nchan` fused FM chains (rr_fm_chain_create) fed by ONE input stream — the reference's Tee fan-out
 * (src/tee.rs:10-24) plus nchan x {FftFilter, RationalResampler, QuadratureDemod}.  taps =
 * [nchan][ntaps] (each channel its own, e.g. the prototype shifted to the channel centre); every
 * tile's forward FFT is computed once for all channels.  The block has nchan OUTPUT windows:
 * rr_block_work[_dev] takes `out` as nchan consecutive windows of out_cap elements (channel c at
 * out + c*out_cap) and reports the per-channel consumed/produced (identical for all channels).
 * Up to 4094 taps the channels share every tile's forward transform in one kernel; longer filters (the reference has no
 * limit) run as one rr_fm_chain per channel on the shared window behind the same handle.  atan2_mode as rr_fm_chain_create. */
rr_block *rr_fm_multi_create(const rr_c32 *taps, size_t nchan, size_t ntaps, size_t interp, size_t deci,
                             float gain, int atan2_mode);
/* The same fed by the RTL-SDR byte stream: RtlSdrDecode (src/rtlsdr_decode.rs:9-47) fused in front of the Tee, as in
 * rr_fm_chain_u8_create (input windows, `consumed` and the WAIT_SRC `need` count BYTES). */
rr_block *rr_fm_multi_u8_create(const rr_c32 *taps, size_t nchan, size_t ntaps, size_t interp, size_t deci,
                                float gain, int atan2_mode);
/* Channelizer: `nchan` FftFilter -> RationalResampler pairs fed by ONE Complex input stream, with Complex (baseband)
 * outputs — the reference's Tee fan-out (src/tee.rs:10-24) plus nchan x {FftFilter::new(_, taps_c)
 * (src/fft_filter.rs:289-355), RationalResampler::new(_, interp, deci) (src/rational_resampler.rs:154-213)}, the front end
 * of examples/rtl_downsampled.rs:37-52, rtl_data_stream.rs:188-205, burst_saver.rs:97-107 and ax25-9600-rx.rs:147-151.
 * taps = [nchan][ntaps].  Whole-stream output of channel c equals the two blocks in sequence, including FftFilter's
 * zero history at the start of the stream and the gcd reduction of interp:deci.  nchan 1 is the fused
 * FftFilter -> RationalResampler block (one output window; rr_block_work_streams takes it).
 * Output windows as rr_fm_multi_create: nchan consecutive windows of out_cap Complex elements, identical counts.
 * Every tile's forward transform is shared by all channels (the kernels of rr_fm_multi_create with the samples stored
 * instead of demodulated).
 * work(): after filtered samples y, N2(y) = ceil(y interp / deci) resampled ones exist.  WAIT_DST(n) when the next filter
 * block's n resampled samples do not fit, else consumes like FftFilter (whole pending blocks) and returns
 * WAIT_SRC(nsamples - pending).  The output window must hold one filter block's worth, ceil(nsamples * interp / deci)
 * (with the reference's 4,096,000-byte streams any ratio up to interp/deci ~ 30 at 16384-point blocks); a smaller one
 * returns WAIT_DST(n) forever.  No tap-count or ratio limit: shapes beyond the fused kernels (more than 4094 taps off the
 * decimate-first tiles, a decimation beyond a tile) run as one FftFilter -> RationalResampler pair of GPU blocks per
 * channel behind the same handle.  NULL + rr_last_error for interp or deci 0 ("RationalResampler created using deci 0"),
 * nchan 0 or above 4096, ntaps 0.  Tags: RR_TAGS_DROP (the resampler drops them, rational_resampler.rs:156).
 * A NaN input sample makes exactly the reference's outputs NaN (the resampled samples of its poisoned FftFilter blocks). */
rr_block *rr_channelizer_create(const rr_c32 *taps, size_t nchan, size_t ntaps, size_t interp, size_t deci);
/* The same fed by the RTL-SDR byte stream: RtlSdrDecode (src/rtlsdr_decode.rs:9-47) fused in front of the Tee, as in
 * rr_fm_multi_u8_create (input windows, `consumed` and the WAIT_SRC `need` count BYTES). */
rr_block *rr_channelizer_u8_create(const rr_c32 *taps, size_t nchan, size_t ntaps, size_t interp, size_t deci);
/* N-station FM receiver down to audio: the whole of examples/rtl_fm.rs:381-419 on every branch of a Tee (src/tee.rs:10-24)
 * fed by ONE Complex input stream — per channel c the six blocks
 *   FftFilter::new(_, rf_taps[c]) (src/fft_filter.rs:289-355) -> RationalResampler::new(_, rf_interp, rf_deci)
 *   (src/rational_resampler.rs:125-206) -> QuadratureDemod::new(_, gain) (src/quadrature_demod.rs:65-109; FastFM
 *   :144-165 with RR_DEMOD_FASTFM) -> FftFilterFloat::new(_, audio_taps) (src/fft_filter.rs:365-491) ->
 *   RationalResampler::new(_, audio_interp, audio_deci) -> MultiplyConst::new(_, scale) (src/multiply_const.rs:6-23)
 * i.e. rr_fm_multi_create followed by one rr_audio_chain_create per channel, as ONE block of two tile launches per call
 * whatever nchan is.  rf_taps = [nchan][rf_ntaps]; audio_taps is one set shared by all channels, as in rtl_fm.  Both filters
 * start from zero history, both ratios are gcd-reduced.  Output: nchan consecutive windows of out_cap f32 elements (channel c
 * at out + c*out_cap), identical counts; rr_block_out_windows returns nchan.
 * work(): no output tail.  With S1 / S2 the nsamples of the RF / audio filter, d(y) = max(ceil(y rf_interp / rf_deci) - 1, 0)
 * the demodulated samples after y filtered ones, and A(k) = ceil(floor(d(k S1) / S2) S2 audio_interp / audio_deci) the audio
 * samples after k RF blocks (K blocks run so far, `pend` input samples carried): WAIT_DST(A(K+1) - A(K)) consuming nothing when
 * that does not fit out_cap; else with k_out the largest k for which A(K+k) - A(K) fits and k_in = floor((pend + len) / S1):
 * k_in > k_out runs k_out blocks, consumes k_out S1 - pend and returns WAIT_DST(A(K+k_out+1) - A(K+k_out)); otherwise runs k_in
 * blocks, consumes the whole window and returns WAIT_SRC(S1 - new pend).  Counts depend on lengths only and are final on
 * return.  EOF follows the source; tags: RR_TAGS_DROP.
 * Shapes beyond the fused kernels (RR_DEMOD_FASTFM, more than 3584 audio taps, RF shapes rr_fm_multi_create runs per channel)
 * run behind the same handle as rr_fm_multi feeding one rr_audio_chain per channel through device-resident streams of the
 * reference's capacity: the same whole-stream output, with the window protocol of that composition (progress on any window,
 * WAIT_DST / WAIT_SRC from the stage that stalls) instead of the one above.
 * NULL + rr_last_error for an interp or deci of 0 ("RationalResampler created using deci 0"), nchan 0 or above 4096, either
 * tap count 0.  A NaN input sample makes exactly the reference's audio samples NaN: those of the audio blocks that hold a
 * demodulated sample of its poisoned RF block. */
rr_block *rr_fm_receiver_create(const rr_c32 *rf_taps, size_t nchan, size_t rf_ntaps, size_t rf_interp, size_t rf_deci,
                                float gain, int atan2_mode, const float *audio_taps, size_t audio_ntaps,
                                size_t audio_interp, size_t audio_deci, float scale);
/* The same fed by the RTL-SDR byte stream: RtlSdrDecode (src/rtlsdr_decode.rs:9-47) fused in front of the Tee — the whole
 * of examples/rtl_fm.rs:328-419 — as rr_fm_multi_u8_create (input windows, `consumed` and the WAIT_SRC `need` count BYTES). */
rr_block *rr_fm_receiver_u8_create(const rr_c32 *rf_taps, size_t nchan, size_t rf_ntaps, size_t rf_interp, size_t rf_deci,
                                   float gain, int atan2_mode, const float *audio_taps, size_t audio_ntaps,
                                   size_t audio_interp, size_t audio_deci, float scale);
/* number of output windows of a block (1 except rr_fm_multi[_u8]_create, rr_channelizer[_u8]_create and rr_fm_receiver[_u8]_create) */
size_t rr_block_out_windows(const rr_block *b);

void rr_block_destroy(rr_block *b);

/* ---- Block trait -------------------------------------------------------------- */
/* Block::work() (src/block.rs:115-126) over the stream windows the Rust shim
 * obtained from `self.src.read_buf()` / `self.dst.write_buf()`
 * (src/stream.rs:208-217, 301-310): `in`/`out` are HOST pointers to contiguous
 * windows of in_len / out_cap ELEMENTS.  The block copies the window to the
 * GPU, runs its HIP kernels and copies the produced samples back before
 * returning.  `*consumed` / `*produced` are what the shim must pass to
 * `consume()` / `produce()`; on RR_WAIT_* `*need` is the WaitForStream amount.
 * Thresholds and return codes follow each block's reference `work()` exactly
 * (src/fir.rs:492-550, src/fft_filter.rs:290-354,
 * src/rational_resampler.rs:155-206, src/quadrature_demod.rs:46-113,
 * src/hilbert.rs:72-128). */
int rr_block_work(rr_block *b, const void *in, size_t in_len, void *out, size_t out_cap,
                  size_t *consumed, size_t *produced, size_t *need);

/* Same contract with DEVICE pointers (device-resident streams between GPU
 * blocks: no PCIe hop).  Kernels are enqueued on `hip_stream` exactly as given (a
 * hipStream_t; NULL = HIP's default stream, which is also what PyTorch's default stream
 * is), so they are ordered with the caller's other work on that stream.  The call returns
 * without waiting; counts are final on return (they depend on lengths only). */
int rr_block_work_dev(rr_block *b, const void *d_in, size_t in_len, void *d_out, size_t out_cap,
                      size_t *consumed, size_t *produced, size_t *need, void *hip_stream);

/* BlockEOF::eof() (src/block.rs:103-110): `src_eof` = all input streams are at
 * EOF; the resampler additionally requires no pending sample
 * (src/rational_resampler.rs:209-213). */
int         rr_block_eof(rr_block *b, int src_eof);
/* BlockName::block_name() (src/block.rs:91-97). */
const char *rr_block_name(const rr_block *b);

/* What the reference block(s) behind this handle do with stream tags (src/stream.rs:48-93).  Tags never cross the
 * C ABI: the shim keeps them on the host and re-bases them from `consumed` / `produced`.  This call
 * tells a GENERIC shim block (GpuResident, GpuFused: one type for every handle) which of the reference's rules
 * applies, in whole-stream positions — a tag on input sample a (counted from the start of the stream):
 *   RR_TAGS_DROP     not forwarded: RationalResampler (rational_resampler.rs:156), QuadratureDemod
 *                    (quadrature_demod.rs:46-113), RtlSdrDecode (rtlsdr_decode.rs:21), every chain containing one.
 *   RR_TAGS_FORWARD  re-emitted on output sample a / *param (integer division) once that output exists:
 *                    FirFilter `pos < n` kept at `pos / deci` (fir.rs:536-545; every window starts at a multiple
 *                    of deci, so the window-relative rule is this one), *param = deci; FftFilter / FftFilterFloat
 *                    (fft_filter.rs:307-313,343 / :441-445,467-472), Hilbert (hilbert.rs:119-123), MultiplyConst,
 *                    FastFM (the sync macro, rustradio_macros_code/src/lib.rs:458-515): *param = 1; the fused
 *                    FirFilter -> FftFilter: 1; Hilbert -> FirFilter(deci): deci.
 *   RR_TAGS_FRAMES   input tags dropped, frame tags added per *param = frame size outputs: FftStream
 *                    (fft_stream.rs:98-111).
 *   RR_TAGS_SHIFT    re-emitted on output sample a + *param once that output exists: Delay (delay.rs:104-108: the copy
 *                    keeps a tag's position in the window, and *param = delay outputs precede the first copied one).
 * Returns the rule, or RR_ERR for a NULL handle. */
enum rr_tag_rule { RR_TAGS_DROP = 0, RR_TAGS_FORWARD = 1, RR_TAGS_FRAMES = 2, RR_TAGS_SHIFT = 3 };
int rr_block_tag_rule(const rr_block *b, size_t *param);
size_t      rr_block_in_elem_size(const rr_block *b);
size_t      rr_block_out_elem_size(const rr_block *b);
/* Wait for everything the block enqueued (its private stream and the stream of the last work call). */
int         rr_block_sync(rr_block *b);

/* Page-lock a host range the library will be handed windows of (hipHostRegister): the reference's stream
 * ring is one stable mapping (src/nowasm/circular_buffer.rs:98-128: base, 2 x len), so the shim registers
 * it once at stream creation.  rr_block_work on windows inside registered ranges then runs ZERO-COPY
 * (round 4): the kernels read the input window and write the output window over PCIe themselves, so the
 * window going down overlaps the one coming up on the full-duplex link — two DMA copies do not on this
 * pool (4,096,000-byte windows: FftFilter 193 -> 148 us per call, the fused RTL-SDR chain 175 -> 109);
 * rr_dstream_copy_in/out on such windows run as copy KERNELS on the range's device view (55 GB/s either way; hipMemcpyAsync
 * gets 16-18 GB/s up and 50 down out of a registered range here: profiles/r05_pcie_inplace.txt).  Windows
 * that are not WHOLLY inside a range registered here (pageable memory, memory the caller page-locked by
 * other means) are staged through device memory — and since round 6 through pinned chunks the library owns,
 * copied by the CPU: no GPU engine is ever pointed at memory the caller did not register (csrc/stage.hpp: the
 * runtime's own pinning of a recycled pageable address was the abort() of rounds 4-5).  Expect one host core's
 * memcpy rate there.  Optional; unregister before the memory is unmapped, and not while a work call on one of
 * its windows is running.
 * Zero-copy is granted only to a range whose base and size are multiples of the SYSTEM page size (sysconf(_SC_PAGESIZE)) and none of
 * whose pages is, or ever was, part of another registration in this process — the reference's ring qualifies
 * (one page-aligned mmap, registered once).  Any other range is still page-locked (its staged copies run as
 * direct DMA) but is never handed to kernels in place: kernels working in place on pages that had been
 * page-locked, released and page-locked again were seen to miss on this platform (csrc/blocks.cpp "WHICH ranges
 * run zero-copy").  RR_ZERO_COPY=0 in the environment turns the in-place path off altogether. */
int rr_host_register(void *ptr, size_t bytes);
/* 1 when rr_block_work would let kernels work IN PLACE on the host window [ptr, ptr + bytes), 0 when it would be staged
 * through device memory (tests assert the path they mean to exercise; a shim can log it once per ring). */
int rr_host_window_in_place(const void *ptr, size_t bytes);
int rr_host_unregister(void *ptr);

/* ---- device-resident streams ----------------------------------------------------------
 * A stream ring in HBM with the reference's window contract (src/stream.rs:187-310 over
 * src/nowasm/circular_buffer.rs:98-128): read window = ALL readable elements, write window = ALL free
 * space, both contiguous (double mapping); capacity in bytes (the reference default is 4,096,000, src/stream.rs:105).
 * GPU blocks chained through these never cross PCIe and never wait for each other: all counts are
 * host-side, kernels and the occasional ring move are enqueued on the caller's HIP stream. */
typedef struct rr_dstream rr_dstream;
rr_dstream *rr_dstream_create(size_t elem_size, size_t capacity_bytes);          /* new_stream(), stream.rs:336-339 */
void        rr_dstream_destroy(rr_dstream *s);
size_t      rr_dstream_capacity(const rr_dstream *s);                            /* elements */
/* 1: the ring is one physical allocation mapped twice back to back (HIP virtual-memory API), the
 * reference's own trick (circular_buffer.rs:98-128), no data is ever moved; 0: linear fallback */
int         rr_dstream_is_double_mapped(const rr_dstream *s);
/* ReadStream::read_buf() (stream.rs:208-217): returns the readable element count, *dev_ptr = window */
size_t      rr_dstream_read_buf(rr_dstream *s, const void **dev_ptr);
/* WriteStream::write_buf() (stream.rs:301-310): returns the free element count, *dev_ptr = window (NULL: the count only) */
size_t      rr_dstream_write_buf(rr_dstream *s, void **dev_ptr, void *hip_stream);
int         rr_dstream_consume(rr_dstream *s, size_t n);                         /* BufferReader::consume */
int         rr_dstream_produce(rr_dstream *s, size_t n);                         /* BufferWriter::produce */
/* The two ends of a stream, and how a graph ENDS (round 4).  The reference's ReadStream / WriteStream share one
 * Arc'd buffer; an end is "closed" when the other end has been dropped (strong count 1: src/stream.rs:148-150,166-168),
 * ReadStream::eof() = writer gone AND ring empty (:237-246), and StreamWait::wait(need) returns true when `need` can
 * never be met (:222-224,311-313) — the three facts Graph::run (src/graph.rs:126-147) and MTGraph (src/mtgraph.rs:98-116)
 * finish a block on.  A shim holds one rr_dstream behind a writer handle and a reader handle, calls rr_dstream_close(s, side)
 * when it drops one of them, and destroys the ring with the last.  Every rr_dstream_* call and rr_block_work_streams
 * takes the ring's own lock, so the two ends may live on different threads (one thread per end). */
enum { RR_SIDE_WRITER = 0, RR_SIDE_READER = 1 };
int         rr_dstream_close(rr_dstream *s, int side);                           /* Drop of that end */
int         rr_dstream_closed(rr_dstream *s, int side);                          /* 1 once `side` has been dropped */
/* StreamWait::wait(need) for the `side` end: blocks until `need` elements are readable (READER) / free (WRITER), the
 * other end closes, or `timeout_ms` passes; returns the count it saw last and sets *never (may be NULL) to 1 when that is
 * below `need` and the other end is closed, i.e. the block should go ahead and EOF. */
size_t      rr_dstream_wait(rr_dstream *s, int side, size_t need, unsigned timeout_ms, int *never);
size_t      rr_dstream_id(const rr_dstream *s);                                  /* StreamWait::id(), shared by both ends */
/* Streams: every call that takes a ring and a `hip_stream` may use its own stream — a source pushing window k + 1 on a copy
 * stream while the blocks of window k run on a compute stream.  The ring orders them (an event from the last writer, and
 * from every stream that read since, before a write; from the last writer before a read); with one stream driving a ring it
 * costs nothing.  rr_dstream_read_buf hands out a raw window without a stream: callers that launch their own work on it are
 * ordered like a block if they go through rr_block_work_streams, and on their own otherwise. */
/* BufferWriter::fill_from_slice from HOST memory into the write window at `offset` (not yet produced).  `host` is the
 * caller's again on return (the call waits for the DMA out of a page-locked ring), so the source window can be consumed
 * and overwritten straight away. */
int         rr_dstream_copy_in(rr_dstream *s, size_t offset, const void *host, size_t n, void *hip_stream);
/* copy `n` elements at `offset` of the read window to HOST memory; waits for the stream (data valid on return) */
int         rr_dstream_copy_out(rr_dstream *s, size_t offset, void *host, size_t n, void *hip_stream);
/* `n` elements at `src_offset` of src's READ window -> dst's WRITE window at `dst_offset` (not yet produced), device to
 * device on `hip_stream`, no host involvement: what Tee (src/tee.rs:10-24) and a ring-to-ring copy need between two HBM rings */
int         rr_dstream_copy(rr_dstream *dst, size_t dst_offset, rr_dstream *src, size_t src_offset, size_t n, void *hip_stream);
/* One Block::work() between two device streams: rr_block_work_dev over their windows + consume/produce. */
int rr_block_work_streams(rr_block *b, rr_dstream *src, rr_dstream *dst, size_t *consumed, size_t *produced,
                          size_t *need, void *hip_stream);

/* ---- multi-GPU fan-out of a shared source ------------------------------------------------------------------
 * One process per GPU, chains sharded by channel; the only exchange is the source, which the reference fans out with a Tee
 * tree inside one process (src/tee.rs:10-24).  An rr_fanout is a double buffer of `tile_bytes` in HBM on every rank plus a
 * communication stream: the owning rank's source block writes tile t into one half, an RCCL broadcast (xGMI) delivers it
 * into the same half on every other rank while the blocks of every rank still read tile t - 1 from the other half.  All
 * ordering is by HIP events between the caller's streams and the communication stream; no call blocks the host.
 *
 *     id:  rank src calls rr_fanout_unique_id and ships the 128 bytes to the other processes (file, socket, MPI, env)
 *     f = rr_fanout_create(id, rank, world, src, tile_bytes, 0)                  -- collective: every rank calls it
 *     per tile t = 0, 1, 2 …, on every rank, in order:
 *         rank src:  p = rr_fanout_produce_buf(f, t, s_src);  … enqueue the source's writes of tile t to p on s_src …
 *         rr_fanout_submit(f, t, s_src)                      -- collective: broadcast of tile t on the communication stream
 *         x = rr_fanout_acquire(f, t, s_blk);  rr_block_work_dev(b, x, …, s_blk) …;  rr_fanout_release(f, t, s_blk)
 *     submit(t + 1) may (and for overlap should) be called before acquire(t); tile t + 2 needs release(t) first.
 *     release(t) is called ONCE per tile, on the one stream that has (transitively) waited for every reader of the tile:
 *     blocks reading a tile on several streams join them into one (hipStreamWaitEvent) before the release — a second
 *     release of the same tile, or one of a tile that has left the double buffer, is an error.
 * A one-rank fan-out (world 1) needs neither an id nor RCCL and keeps the same calls, so a graph is written once.
 * RCCL is bound at run time (dlopen), the library itself does not depend on it.  Like a block, a handle is driven by one
 * thread at a time; calls made out of protocol order (a tile skipped, a half not yet released) fail with RR_ERR / NULL and
 * rr_last_error instead of racing. */
typedef struct rr_fanout rr_fanout;
#define RR_FANOUT_ID_BYTES 128
enum rr_fanout_flags {
    RR_FANOUT_TIMING      = 1,  /* time every 4th broadcast with HIP events on the communication stream (rr_fanout_stats) */
    RR_FANOUT_RCCL_ALWAYS = 2,  /* run a one-rank group through RCCL as well (tests of the RCCL path on a one-GPU machine) */
    RR_FANOUT_MESH        = 4   /* fan out by ncclScatter (1/world of the tile to each rank) + in-place ncclAllGather between the
                                   receivers instead of one ncclBroadcast: a broadcast is bounded by ONE of the owner's xGMI
                                   links, this form spreads the tile over the full mesh (same flag on every rank) */
};
int         rr_fanout_unique_id(void *id128);
rr_fanout  *rr_fanout_create(const void *id128, int rank, int world, int src_rank, size_t tile_bytes, int flags);
void        rr_fanout_destroy(rr_fanout *f);
void       *rr_fanout_produce_buf(rr_fanout *f, unsigned long long t, void *producer_stream);   /* NULL + rr_last_error */
int         rr_fanout_submit(rr_fanout *f, unsigned long long t, void *producer_stream);        /* non-owning ranks: stream unused */
const void *rr_fanout_acquire(rr_fanout *f, unsigned long long t, void *compute_stream);        /* NULL + rr_last_error */
int         rr_fanout_release(rr_fanout *f, unsigned long long t, void *compute_stream);
/* waits for the communication stream; summed duration and number of the broadcasts timed since the last call */
int         rr_fanout_stats(rr_fanout *f, double *broadcast_ms, size_t *broadcasts);

/* ---- KISS framing on the device (src/kiss.rs) -------------------------------------------------------------------
 * The host side of examples/bell202.rs and examples/g3ruh.rs: ReaderSource -> KissFrame -> KissDecode -> FcsAdder -> … on the way
 * out, … -> HdlcDeframer -> KissEncode -> PduToStream -> WriterSink on the way in.  FEND 0xC0, FESC 0xDB, TFEND 0xDC, TFESC 0xDD
 * (:7-10).  Batch blocks: rr_block_work on either handle is an error.
 *
 * rr_kiss_decode: KissFrame (:165-228) -> KissDecode (:96-137) over pushes of one byte stream, in closed form.  With f_0 < f_1 < …
 * the positions of the stream's FEND bytes: bytes in front of f_0 are dropped (Unsynced); every gap G = b[f_j + 1 .. f_j+1) with
 * 1 <= |G| <= max_len is one KissFrame output (an empty gap is none, :204-206; a longer one is none and the machine resyncs at
 * f_j+1, :211-217); G[0] & 0x0F != 0 drops it as non-data (:110-113), else port = G[0] >> 4 and x = G[1..] is un-escaped
 * (:47-77): x is dropped when some FESC of it is its last byte or is followed by a byte other than TFEND / TFESC, else the packet
 * is x without its FESC bytes, the byte behind each mapped TFEND -> FEND, TFESC -> FESC.  A packet of 0 bytes is delivered.  The
 * three tags (:122-134) are record fields.  A push delivers every packet whose closing FEND lies inside it, whatever the split of
 * the stream into pushes; the dst.remaining() back-pressure (:99-101, :168-170) has no counterpart.  The state between pushes —
 * whether a FEND has been seen, the bytes of the gap still open (at most max_len = carry_bytes; a longer open gap carries
 * nothing) and the five counters — stays on the device.  max_len 10000 is the reference's MAX_LEN (:6).
 * NULL + rr_last_error, said before any device is touched: "kiss decode: max_len out of range (1 .. 2^20)". */
typedef struct {
    unsigned long long pos;    /* stream position of the closing FEND */
    unsigned long long start;  /* first byte of the packet in the byte arena of this push; packets lie packed in stream order */
    unsigned len;              /* "KissDecode:output-bytes" */
    unsigned in_bytes;         /* "KissDecode:input-bytes": |x|, the escaped bytes behind the port byte */
    unsigned port;             /* "KissDecode:port" */
    unsigned reserved;         /* 0 */
} rr_kiss_packet;              /* 32 bytes */
rr_block *rr_kiss_decode_create(size_t max_len);
/* The next n bytes of the stream, on the device (read on hip_stream) or on the host.  n == 0 launches nothing and leaves every
 * state alone.  RR_ERR before any device is touched, nothing launched: "kiss decode: null input", "kiss decode: more than 2^30
 * bytes in one push". */
int rr_kiss_decode_push_dev(rr_block *b, const void *d_bytes, size_t n, void *hip_stream);
int rr_kiss_decode_push(rr_block *b, const unsigned char *bytes, size_t n);
/* The packets of the most recent push, ascending by pos (the contract of rr_wpcr_results), and their bytes.  Both wait for the
 * push; every number the device wrote is checked against the push's length, the carry bound and max_len before it is used. */
int rr_kiss_packets(rr_block *b, rr_kiss_packet *rec, size_t cap, size_t *total);
int rr_kiss_packet_bytes(rr_block *b, unsigned char *out, size_t cap, size_t *total);
/* The arena of the most recent push on the device (valid until the next push); *n_total: an upper bound of its bytes. */
const void *rr_kiss_packet_bytes_dev(rr_block *b, size_t *n_total);
/* So far: KissFrame outputs, packets delivered, non-data frames, bad escapes, gaps of more than max_len bytes (counted at the FEND
 * that closes them).  frames = delivered + nondata + bad_escape. */
int rr_kiss_decode_stats(rr_block *b, unsigned long long *five);
/* The tile in bytes, the most bytes a push carries over, and the kernel launches of every push of n > 0 bytes. */
int rr_kiss_decode_dims(const rr_block *b, size_t *tile_bytes, size_t *carry_bytes, size_t *launches);

/* rr_kiss_encode: KissEncode (:247-286) -> PduToStream over a batch of packets of one byte buffer: per packet FEND, port << 4, the
 * bytes with FEND -> FESC TFEND and FESC -> FESC TFESC (escape, :30-44), FEND; the frames lie back to back in d_out.  A port of
 * 16 or more is 0 (:261-265).  The port byte is NOT escaped, as in the reference: port 12 writes a raw 0xC0. */
typedef struct {
    size_t start, len;         /* the frame is d_out[start .. start + len): "KissEncode:output-bytes" */
    unsigned escaped;          /* len = 3 + L + escaped, L = the packet's bytes ("KissEncode:input-bytes") */
    unsigned port;
} rr_kiss_frame_record;
rr_block *rr_kiss_encode_create(void);
/* sum of 3 + 2 L: what out_cap must hold.  Saturates at SIZE_MAX. */
size_t rr_kiss_encode_bound(const size_t *lens, size_t npackets);
/* Packet p is bytes[starts[p] .. starts[p] + lens[p]) (ranges may overlap or repeat), its port ports[p] (NULL: 0).  npackets == 0
 * launches nothing.  RR_ERR before any device is touched, nothing launched: "kiss encode: null packet descriptors", "… more than
 * 2^30 bytes in one push", "… packet outside the buffer", "… more than 2^30 encoded bytes in one push", "… output shorter than the
 * encoded bytes can be", "… null argument".  Bytes of d_out beyond *produced are not written. */
int rr_kiss_encode_push_dev(rr_block *b, const void *d_bytes, size_t n_bytes, size_t *starts, size_t *lens, const unsigned *ports,
                            size_t npackets, void *d_out, size_t out_cap, void *hip_stream);
int rr_kiss_encode_push(rr_block *b, const unsigned char *bytes, size_t n_bytes, size_t *starts, size_t *lens, const unsigned *ports,
                        size_t npackets, unsigned char *out, size_t out_cap, size_t *produced);
/* The frames of the most recent push (the contract of rr_wpcr_results) and their sum; waits for the push. */
int rr_kiss_encode_records(rr_block *b, rr_kiss_frame_record *rec, size_t cap, size_t *total, size_t *produced);
int rr_kiss_encode_dims(const rr_block *b, size_t *tile_bytes, size_t *launches);
/* The two joins, in the manner of rr_wpcr_process_pdus: wait for the producer's most recent push, take its checked records on the
 * host, run the consumer on the producer's device arena — the payload bytes never leave the device.
 * rr_kiss_encode_frames: the frames of an rr_hdlc_deframer (port 0; port_of_stream may be NULL) or an rr_hdlc_receiver (port
 * port_of_stream[rec.stream], nports >= its streams) -> KISS bytes in d_out; any other handle is RR_ERR.
 * rr_hdlc_framer_push_kiss: the packets of an rr_kiss_decode -> rr_hdlc_framer_push_dev. */
int rr_kiss_encode_frames(rr_block *kiss, rr_block *deframer_or_receiver, const unsigned *port_of_stream, size_t nports, void *d_out,
                          size_t out_cap, void *hip_stream);
int rr_hdlc_framer_push_kiss(rr_block *framer, rr_block *kiss_decode, void *d_out, size_t out_cap, void *hip_stream);

/* Measurement aid: when enabled, every work call brackets the block's dominant kernel
 * with HIP events on the stream it is launched on; rr_block_profile waits for them and
 * returns the summed kernel time and the number of launches (reset != 0 clears them). */
int rr_block_set_profiling(rr_block *b, int on);
int rr_block_profile(rr_block *b, double *total_ms, size_t *launches, int reset);

/* Measurement builds only (make TIMING=1): 32 s_memtime stamps taken at the phase boundaries of one tile of the
 * last stamped kernel (out must hold 32 values); returns 0 in product builds. */
int rr_debug_fft_stamps(unsigned long long *out32);
/* Kernel launches the library has made in this process so far (every hipLaunchKernelGGL of a block's work(), incl. carry
 * copies and repair passes; not the copies of host windows).  Tests use the difference around one call: a clean
 * FftFilter work() on a device window is ONE launch (round 6; the reference's one work() = one pass over the window,
 * src/fft_filter.rs:289-355). */
unsigned long long rr_debug_kernel_launches(void);
/* Introspection for tests: the kernel family of the handle's most recent EMITTING work() call, for the blocks that pick
 * their kernel per call by the size of the window (the fused FM chains, FftFilter / FirFilter -> FftFilter, Hilbert ->
 * FirFilter, FirFilter<Complex>).  A static string, one of "poly" (decimate-first tiles), "half" (half-size inverse), "alt" (plain 4096-point
 * tile of a long filter), "split" (8192 / 16384-point split tile), "full" (plain tile), "prune" (pruned inverse),
 * "direct" (direct form), "two-stage" (two kernels through a work buffer), "deci" (tiles with a decimating store).
 * "" for a block without such a choice, for a handle that has not emitted yet and for NULL.  The result of work() does
 * not depend on the family beyond f32 rounding; tests use it to prove that a schedule of windows really switched. */
const char *rr_debug_last_kernel(const rr_block *b);
/* Introspection for tests: the f32 magnitudes mag[0 .. N / 2) that rr_wpcr's decision for burst `burst` of the most recent
 * process call was taken on (the device keeps them anyway).  Waits for that call; writes the first min(*nbins, cap) of them,
 * *nbins = N / 2 (0 for a burst shorter than 2 samples). */
int rr_debug_wpcr_spectrum(rr_block *b, size_t burst, float *mag, size_t cap, size_t *nbins);
/* Introspection for tests: the two elements Midpointer's offset of PDU idx of the most recent push was made of — `low`, the
 * element of rank nlow / 2, and `high`, the element of rank nlow + (len - nlow) / 2 (both 0 for a PDU with ok == 0).  Waits for
 * that push.  RR_ERR for a handle without RR_PDU_MIDPOINT and for an idx beyond the push's PDUs. */
int rr_debug_pdu_ranks(rr_block *b, size_t idx, float *low, float *high);

/* ---- per-block knobs / introspection ------------------------------------------- */
/* FftFilter: reference fft_size and nsamples (src/fft_filter.rs:261-262) and the
 * internal overlap-save tile the GPU kernel uses. */
int rr_fftfilter_dims(const rr_block *b, size_t *fft_size, size_t *nsamples, size_t *gpu_fft_size);
/* FirFilter<Complex>: size of the overlap-save FFT tile a non-decimating filter runs on, 0 when the block uses the
 * direct-form kernel (introspection for tests and benches; the result of Fir::filter, src/fir.rs:166-197, either way). */
size_t rr_fir_fft_tile(const rr_block *b);
/* FirFilter translate (also inside rr_hilbert_fir_create): rotator mode (default RR_ROT_REPLAY, the on-parity one).
 * Switching to a REPLAY mode after outputs were produced walks the chain from the stream start first (once). */
int rr_fir_set_rotator_mode(rr_block *b, int mode);

#ifdef __cplusplus
}
#endif
#endif /* RUSTRADIO_AMD_H */
