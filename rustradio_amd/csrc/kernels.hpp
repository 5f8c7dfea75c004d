// kernels.hpp — host-callable launchers of the HIP kernels (one TU per kernel family).
#pragma once
#include "common.hpp"
#include "hdlc_dims.hpp"
#include "il2p_core.hpp"
#include "nan_fix.hpp"
#include "pwm_core.hpp"
#include "symsync_core.hpp"
#include "afsk_core.hpp"
#include "am_core.hpp"
#include "fsk_core.hpp"

namespace rr {

// ---- kernels_fft.hip ---------------------------------------------------------------
// Overlap-save FFT filter.  xx = virtual stream whose index 0 is the first of the
// (L-1) history samples.  Writes y[n] = sum_k t[k] * x[n - k], n < n_out, where x[i] = xx[i + L - 1].
//   log2f      : internal tile size F = 2^log2f (10..14), F >= 2*(L-1) recommended
//   tw         : device table of w_F^k, k < F
//   hpos       : device table of H (scaled by 1/F) in digit-reversed position order
bool fftfilt_supported(int log2f);
int fft_read_stamps(unsigned long long* host16);   // measurement builds only (else returns 0)
// (carry: the caller's carry-state update, done by this launch — every launcher below that takes one falls back to a
//  separate copy kernel when it has nothing to launch)
// (fx: FirFilter on these tiles — non-finite input samples get the reference's locality, nan_fix.hpp; default: none)
void launch_fftfilt_os(int log2f, VSrc<cf> src, cf* out, long n_out, int L, const cf* tw,
                       const cf* hpos, hipStream_t s, CarryOut carry = {}, NanFix fx = {});

// The same filter keeping every d-th output: out[m] = y[m d], m < n_out (tiles of 1024..4096 points, d <= 4096) —
// the decimating FirFilter (fir.rs:181-189) on overlap-save tiles.
void launch_fftfilt_deci(int log2f, VSrc<cf> src, cf* out, long n_out, int L, int d, const cf* tw, const cf* hpos,
                         hipStream_t s, NanFix fx = {});

// Real stream, real taps (hpos from Complex(t, 0)): out[m] = y[m d], y[n] = sum_k t[k] xx[n + L - 1 - k]; two
// overlap-save segments ride in the real / imaginary lanes of one Complex tile (tiles of 1024..4096 points).
void launch_fftfilt_real_hilbert(int log2f, VSrc<float> src, cf* out, long n_out, int L, const cf* tw, const cf* hpos, hipStream_t s,
                                 CarryOut carry, NanFix fx = {});
void launch_fftfilt_real(int log2f, VSrc<float> src, float* out, long n_out, int L, int d, const cf* tw, const cf* hpos,
                         hipStream_t s, CarryOut carry = {}, NanFix fx = {});

// FftFilterFloat -> RationalResampler(I:D) -> MultiplyConst fused on the real-stream tiles: out[m - r_lo] = scale *
// y[floor(m D / I)] for the resampled samples m in [r_lo, r_hi) whose source lies in this call's y[A .. A + n_y).
struct AudioChainArgs {
    long A, n_y, r_lo, r_hi, I, D;
    float scale;
    CarryOut carry;    // the block's carry-state update, written by this launch (common.hpp)
};
void launch_audio_chain(int log2f, VSrc<float> src, float* out, int L, const cf* tw, const cf* hpos, const AudioChainArgs& a,
                        hipStream_t s);
// The same for C streams of one shape in ONE launch (k_audio_multi, the audio half of rr_fm_receiver_create): stream c is
// VSrc<float>{prefix + c * pstride, plen, in + c * in_stride, in_len}, writes out + c * out_stride, and a.carry.dst is the
// base of C carry prefixes pstride apart.  One filter (tw, hpos) for all streams; the work items are (stream, tile) pairs.
struct AudioMultiSrc {
    const float* prefix; long plen, pstride;
    const float* in; long in_len, in_stride;
};
bool audio_multi_supported(int log2f);
void launch_audio_multi(int log2f, const AudioMultiSrc& src, int C, float* out, long out_stride, int L, const cf* tw, const cf* hpos,
                        const AudioChainArgs& a, hipStream_t s);

// Decimation by D = F / 256 (4 / 8 / 16 on tiles of 1024 / 2048 / 4096 points) with a pruned inverse transform
// (k_fftfilt_prune): out[m] = y[m D], m < n_out.  Tables (see the kernel): hpos2 = H in position order with the
// factors w_D^(-c k3) w_16D^(-c k2), c = (L - 1) % D, folded in; twb[n2 * 16 + k1] = exp(+2 pi i k1 (n2 D + c) / F).
int prune_log2f_for_deci(int d);                 // 0 when d is not 4 / 8 / 16
bool prune_split(size_t d, size_t& D, size_t& sub);   // d = D * sub, D in {16, 8, 4} (the pruned tile), sub <= 64
void launch_fftfilt_prune_c32(int log2f, VSrc<cf> src, cf* out, long n_out, int L, const cf* tw, const cf* hpos2,
                              const cf* twb, hipStream_t s, int sub = 1, NanFix fx = {});
// real stream, real taps, f32 output (decimating FirFilter<Float>)
void launch_fftfilt_prune_f32(int log2f, VSrc<float> src, float* out, long n_out, int L, const cf* tw, const cf* hpos2,
                              const cf* twb, hipStream_t s, int sub = 1, NanFix fx = {});
// real stream, Complex taps t = Gr + i Gi: hpos2r / hpos2i from the real tap sets Gr / Gi; Complex output
void launch_fftfilt_prune_real(int log2f, VSrc<float> src, cf* out, long n_out, int L, const cf* tw, const cf* hpos2r,
                               const cf* hpos2i, const cf* twb, hipStream_t s, CarryOut carry = {}, int sub = 1, NanFix fx = {});

// Even decimations on 2048-point tiles with the half-size inverse (k_fftfilt_half): out[m] = y[m d], m < n_out.
// tw = w_2048^k, tw_half = w_1024^k, hpos = H / F in the 2048-point position order.
bool fftfilt_half_supported(int L, long d);
void launch_fftfilt_half(VSrc<cf> src, cf* out, long n_out, int L, int d, const cf* tw, const cf* tw_half, const cf* hpos,
                         hipStream_t s, NanFix fx = {});

// The same filter with an 8192 / 16384-point tile built from nsub = 2 / 4 sub-transforms of 4096 points
// (k_fftfilt_split).  tw4096: w_4096^k;  wk[t] = w_F^t, t < 256;  hs[r][p] = H[nsub bin(p) + r] / F with
// bin(p) = fftfilt_split_bin(p), the bin at position p of the 4096-point spectrum layout.
void launch_fftfilt_split(int nsub, VSrc<cf> src, cf* out, long n_out, int L, const cf* tw4096, const cf* hs, const cf* wk,
                          hipStream_t s, CarryOut carry = {}, NanFix fx = {});
void launch_fftfilt_split_deci(int nsub, VSrc<cf> src, cf* out, long n_out, int L, int d, const cf* tw4096, const cf* hs,
                               const cf* wk, hipStream_t s, NanFix fx = {});   // out[m] = y[m d], m < n_out
int fftfilt_split_bin(int p);

// FftStream: out = forward unnormalised FFT of each of `nframes` consecutive 2^log2n-point frames
// (log2n 1..14), natural bin order; tw = device table of w_N^k, k < N.
// (tw4096 = w_4096^k: when given, 8192 / 16384-point frames run as 2 / 4 sub-transforms of 4096 points)
void launch_fft_frames(int log2n, const cf* in, cf* out, long nframes, const cf* tw, const cf* tw4096, hipStream_t s);

// ... of any other size N, 2 N - 1 <= 2^log2m <= 4096, by Bluestein's chirp-z convolution on the filter tile:
// chirp[n] = exp(-i pi n^2 / N), n < N;  hpos = FFT_M(b) / M in position order, b[m] = conj(chirp[|m|]) wrapped mod M.
void launch_fft_bluestein(int log2m, const cf* in, cf* out, long nframes, int N, const cf* tw, const cf* hpos,
                          const cf* chirp, hipStream_t s);

// Fused FftFilter -> RationalResampler -> QuadratureDemod over the same virtual stream.
struct FmChainArgs {
    long A;            // filtered samples emitted before this call
    long n_y;          // filtered samples covered by this call (multiple of the reference nsamples)
    long r_lo, r_hi;   // resampled samples r[m] = y[floor(m*D/I)] whose source lies in [A, A+n_y)
    long o_base;       // demodulated samples emitted before this call
    long I, D;         // reduced interp / deci
    float gain;
    int mode;          // RR_ATAN2_*
    CarryOut carry;    // the block's carry-state update (new prefix), written by this launch (common.hpp)
    int multi_waves = 0;   // multi-channel decimate-first kernel: 0 = by predicted cost, 8 / 12 = that many waves per workgroup
    NanFix fx;             // mode 2 only (launch_fir_poly): nan_fix.hpp
};
// out[(u-1) - o_base] = gain * atan2(conj(r[u-1]) r[u]) for u in [max(r_lo,1), r_hi); r[r_lo-1] is
// *last_in (previous call), r[r_hi-1] is written to *last_out.
void launch_fm_chain(int log2f, VSrc<cf> src, float* out, int L, const cf* tw, const cf* hpos,
                     const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// ... with the RtlSdrDecode conversion fused in front (window = u8 I/Q pairs, carried prefix Complex).
void launch_fm_chain_iq8(int log2f, VSrcIQ8 src, float* out, int L, const cf* tw, const cf* hpos,
                         const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// ... on 8192 / 16384-point tiles built from nsub = 2 / 4 sub-transforms (tables as launch_fftfilt_split)
void launch_fm_chain_split(int nsub, VSrc<cf> src, float* out, int L, const cf* tw4096, const cf* hs, const cf* wk,
                           const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);
void launch_fm_chain_split_iq8(int nsub, VSrcIQ8 src, float* out, int L, const cf* tw4096, const cf* hs, const cf* wk,
                               const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// The same for `nchan` channels that share the input: hpos_all = [nchan][F] frequency responses,
// channel c writes out + c*out_stride and carries last_in[c] / last_out[c].  3-pass tiles (F <= 4096).
bool fm_multi_supported(int log2f);
void launch_fm_multi(int log2f, VSrc<cf> src, float* out, long out_stride, int L, const cf* tw, const cf* hpos_all,
                     int nchan, const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// ... with the RtlSdrDecode conversion fused in front (window = u8 I/Q pairs)
void launch_fm_multi_iq8(int log2f, VSrcIQ8 src, float* out, long out_stride, int L, const cf* tw, const cf* hpos_all,
                         int nchan, const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);
void launch_fm_multi_half_iq8(int log2f, VSrcIQ8 src, float* out, long out_stride, int L, const cf* tw, const cf* tw_half,
                              const cf* hpos_all, int nchan, const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);
// interp 1 and an even decimation on 2048-point tiles: per channel a folded 1024-point inverse on one wave
// (k_fm_multi_half); tw_half = w_(F/2)^k.
bool fm_multi_half_supported(int log2f, long I, long D, int L);
void launch_fm_multi_half(int log2f, VSrc<cf> src, float* out, long out_stride, int L, const cf* tw, const cf* tw_half,
                          const cf* hpos_all, int nchan, const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// the single fused chain on the same half-size inverses (2048-point tiles; fm_multi_half_supported(11, I, D, L))
void launch_fm_chain_half(VSrc<cf> src, float* out, int L, const cf* tw, const cf* tw_half, const cf* hpos,
                          const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);
void launch_fm_chain_half_iq8(VSrcIQ8 src, float* out, int L, const cf* tw, const cf* tw_half, const cf* hpos,
                              const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// ---- kernels_poly.hip: fused FM chains with an integer decimation on decimate-first (polyphase) tiles ----------------
// tw = w_1024^k; hreg = per channel and phase p the response FFT_1024(t[D j + p]) / 1024, register-major:
// hreg[((c D + p) 16 + j) 64 + lane] = H_{c,p}[fm_poly_bin(j, lane)].  a.I must be 1.
bool fm_poly_supported(long I, long D, int L, bool multi);
int fm_poly_bin(int j, int lane);
void launch_fm_chain_poly(VSrc<cf> src, float* out, int L, const cf* tw, const cf* hreg, const FmChainArgs& a, const cf* last_in,
                          cf* last_out, hipStream_t s);
void launch_fm_chain_poly_iq8(VSrcIQ8 src, float* out, int L, const cf* tw, const cf* hreg, const FmChainArgs& a, const cf* last_in,
                              cf* last_out, hipStream_t s);
// decimating FirFilter<Complex> (deci = D) on the decimate-first tiles: out[m] = sum_k t[k] x[m D + L - 1 - k]
void launch_fir_poly(VSrc<cf> src, cf* out, long n_out, int L, int D, const cf* tw, const cf* hreg, hipStream_t s, NanFix fx = {});
void launch_fm_multi_poly(VSrc<cf> src, float* out, long out_stride, int L, const cf* tw, const cf* hreg, int nchan,
                          const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);
void launch_fm_multi_poly_iq8(VSrcIQ8 src, float* out, long out_stride, int L, const cf* tw, const cf* hreg, int nchan,
                              const FmChainArgs& a, const cf* last_in, cf* last_out, hipStream_t s);

// ---- the channelizer (rr_channelizer_create): the multi-channel kernels above with the resampled samples STORED ----------
// Complex out: channel c writes out[c out_stride + u - r_lo] = r[u] for u in [r_lo, r_hi) (a.o_base = a.r_lo); no
// demodulator, no carried r.  Tables and shapes as launch_fm_multi / launch_fm_multi_half / launch_fm_multi_poly.
void launch_chan_multi(int log2f, VSrc<cf> src, cf* out, long out_stride, int L, const cf* tw, const cf* hpos_all, int nchan,
                       const FmChainArgs& a, hipStream_t s);
void launch_chan_multi_iq8(int log2f, VSrcIQ8 src, cf* out, long out_stride, int L, const cf* tw, const cf* hpos_all, int nchan,
                           const FmChainArgs& a, hipStream_t s);
void launch_chan_multi_half(int log2f, VSrc<cf> src, cf* out, long out_stride, int L, const cf* tw, const cf* tw_half,
                            const cf* hpos_all, int nchan, const FmChainArgs& a, hipStream_t s);
void launch_chan_multi_half_iq8(int log2f, VSrcIQ8 src, cf* out, long out_stride, int L, const cf* tw, const cf* tw_half,
                                const cf* hpos_all, int nchan, const FmChainArgs& a, hipStream_t s);
void launch_chan_poly(VSrc<cf> src, cf* out, long out_stride, int L, const cf* tw, const cf* hreg, int nchan, const FmChainArgs& a,
                      hipStream_t s);
void launch_chan_poly_iq8(VSrcIQ8 src, cf* out, long out_stride, int L, const cf* tw, const cf* hreg, int nchan, const FmChainArgs& a,
                          hipStream_t s);

// ---- kernels_fir.hip ---------------------------------------------------------------
struct FirPlan {             // host-prepared polyphase tap table
    int L = 0, d = 1;
    int qpad = 0;            // taps per phase, padded to a multiple of 8
    bool complex_taps = false;
    int cfg = -1;            // >= 0: force tile shape cfg (rr_build_opts.fir_cfg, parity tests of every shape)
};
// y[m] = sum_k rev[k] * x[m*d + k], m < n_out  (rev = reversed taps), x = virtual stream.
// tp = device polyphase table [d][qpad] (float if real taps else cf), rev = device reversed taps.
bool fir_direct_has_tile(const FirPlan& pl, size_t es_in, size_t es_out);   // false: only the slow one-thread-per-output fallback
void launch_fir_c32(const FirPlan& pl, const void* tp, const void* rev, VSrc<cf> src, cf* out,
                    long n_out, hipStream_t s, NanFix fx = {});
void launch_fir_f32(const FirPlan& pl, const float* tp, const float* rev, VSrc<float> src,
                    float* out, long n_out, hipStream_t s, NanFix fx = {});
// Hilbert: out[k] = (xp[k + L/2], sum_j rev[j] xp[k + j]), xp = virtual stream (history ++ in).
// real samples, Complex taps, Complex output (the composite Hilbert -> FirFilter filter)
void launch_fir_f32c(const FirPlan& pl, const cf* tp, const cf* rev, VSrc<float> src, cf* out, long n_out,
                     hipStream_t s, NanFix fx = {});
void launch_hilbert(const FirPlan& pl, const float* tp, const float* rev, VSrc<float> src, cf* out,
                    long n_out, hipStream_t s, NanFix fx = {});
// Hilbert with the zero taps skipped: hq[q] = rev[2q + par] (Q entries, padded to a multiple of 8).
// Returns false if the shape is not covered (use launch_hilbert).
constexpr int HILBERT_MAX_GRID = 8192;        // workgroups k_hilbert is launched with at most (NanFix::wgflags has one word each)
bool launch_hilbert_skip(int L, int par, int Q, const float* hq, VSrc<float> src, cf* out, long n_out, hipStream_t s, NanFix fx = {});
// y[m] *= phase0 * step^(m0 + m) evaluated in f64 (RR_ROT_MODEL)
void launch_rotate_model(cf* y, long n, double p0x, double p0y, double sx, double sy, long m0,
                         hipStream_t s);
// RR_ROT_REPLAY: phase_{i+1} = phase_i * step in f32 (the reference's recurrence) from *state: nskip steps without a store,
// then ring[(pos0 + i) & mask] = phase_i for i < n (mask = ring capacity - 1, a power of two); *state <- the phase after them
void launch_rotor_replay(cf* state, float stx, float sty, cf* ring, long pos0, long mask, long nskip, long n, hipStream_t s);
// y[m] *= ring[(pos0 + m) & mask]
void launch_rotate_table(cf* y, long n, const cf* ring, long pos0, long mask, hipStream_t s);

// ---- kernels_misc.hip --------------------------------------------------------------
// out[r + m] = in[floor((m*D - c0) / I)], m < n_gather; out[0..r) = *pending
void launch_resample(const void* in, void* out, size_t es, long r, const void* pending,
                     long n_gather, long I, long D, long c0, hipStream_t s);
// out[n] = gain * atan2(Im z, Re z), z = conj(x[n]) x[n+1], n < n_out
void launch_quaddemod(const cf* in, float* out, long n_out, float gain, int mode, hipStream_t s);
void launch_mulconst_f32(const float* in, float* out, long n, float v, hipStream_t s);
void launch_mulconst_c32(const cf* in, cf* out, long n, float vr, float vi, hipStream_t s);
// AddConst (add_const.rs:51-68): out[i] = in[i] + v, per component for Complex; bit-exact
void launch_addconst_f32(const float* in, float* out, long n, float v, hipStream_t s);
void launch_addconst_c32(const cf* in, cf* out, long n, float vr, float vi, hipStream_t s);
// FastFM over src = (q2, q1) || window: n outputs
void launch_fastfm(VSrc<cf> src, float* out, long n, hipStream_t s);
// RtlSdrDecode: out[i] = ((in[2i] - 127) * 0.008, (in[2i+1] - 127) * 0.008)
void launch_rtlsdr_decode(const unsigned char* in, cf* out, long n_out, hipStream_t s);
// dst[i] = src.load(v0 + i), i < n   (carry-state update)
void launch_vcopy_c32(VSrc<cf> src, long v0, cf* dst, long n, hipStream_t s);
void launch_vcopy_iq8(VSrcIQ8 src, long v0, cf* dst, long n, hipStream_t s);   // decoding copy
void launch_vcopy_f32(VSrc<float> src, long v0, float* dst, long n, hipStream_t s);
// Hilbert on transform tiles: every non-finite output of a poisoned tile recomputed with the reference's fold (kernels_misc.hip)
void launch_hilbert_refold_nonfinite(VSrc<float> src, cf* out, long n_out, long P, int L, const float* rev, hipStream_t s);
// FftFilter / FftFilterFloat: non-finite samples poison the REFERENCE's blocks, not the GPU's tiles (kernels_misc.hip)
void launch_ref_blocks_nonfinite(VSrc<cf> src, cf* out, long n_out, long S, long P, long hist, int L, int front, const cf* rev, int* tail, int seq, bool force0, hipStream_t s);
void launch_ref_blocks_nonfinite(VSrc<float> src, float* out, long n_out, long S, long P, long hist, int L, int front, const float* rev, int* tail, int seq, bool force0, hipStream_t s);
// the fused FM / audio chains: the same through the resampler's index map and the demodulator's pair (kernels_misc.hip); slots = int[6]
void launch_chain_blocks_nonfinite(VSrc<cf> src, float* out, long out_stride, int nchan, const FmChainArgs& a, long S, long hist, long P,
                                   int L, int front, const cf* rev, long rev_stride, const cf* last_in, cf* last_out, int* slots, int seq, int force,
                                   hipStream_t s);
void launch_chain_blocks_nonfinite(VSrc<float> src, float* out, const AudioChainArgs& a, long S, long hist, long P, int L,
                                   const float* rev, int* slots, int seq, hipStream_t s);
// ... C audio streams of one shape (launch_audio_multi): the stream in the grid, slots = int[C][6], one set of reversed taps
void launch_audio_multi_blocks_nonfinite(const AudioMultiSrc& src, int C, float* out, long out_stride, const AudioChainArgs& a, long S,
                                         long hist, long P, int L, const float* rev, int* slots, int seq, hipStream_t s);
// ... and the channelizer's Complex outputs (out[u - r_lo] = r[u] per channel)
void launch_chan_blocks_nonfinite(VSrc<cf> src, cf* out, long out_stride, int nchan, const FmChainArgs& a, long S, long hist, long P,
                                  int L, const cf* rev, long rev_stride, int* slots, int seq, hipStream_t s);
// a CarryOut as its own launch (calls without a main kernel; launchers with nothing to launch)
void launch_carry(VSrc<cf> src, const CarryOut& c, hipStream_t s);
void launch_carry(VSrcIQ8 src, const CarryOut& c, hipStream_t s);
void launch_carry(VSrc<float> src, const CarryOut& c, hipStream_t s);
void launch_f32_to_c32(const float* in, cf* out, long n, hipStream_t s);
void launch_copy_bytes(const void* src, void* dst, size_t bytes, hipStream_t s);   // device <-> device view of registered host memory
void launch_c32_re(const cf* in, float* out, long n, hipStream_t s);

// ---- kernels_tx.hip: Vco (vco.rs:9-37) as a tiled f64 scan ---------------------------------------------------------------
// out[i] = (sin p_i, cos p_i), p_i = *carry_in + k (a_0 + ... + a_i) modulo 2 pi, i < n; *carry_out <- p_(n-1).  carry_in and
// carry_out are distinct device doubles (the block's ping-pong); tiles = device scratch of ceil(n / VCO_T) doubles.
// n == 0 launches nothing and leaves *carry_out alone.
constexpr int VCO_T = 2048;                   // samples of one scan tile
void launch_vco(const float* in, cf* out, long n, double k, const double* carry_in, double* carry_out, double* tiles, hipStream_t s);
// ... reading its samples through the resampler's index map (launch_resample's r, pending, n_gather, I, D, c0): n = r + n_gather
void launch_fm_tx(const float* in, cf* out, long r, const float* pending, long n_gather, long I, long D, long c0, double k,
                  const double* carry_in, double* carry_out, double* tiles, hipStream_t s);

// ---- kernels_tx.hip: rr_fsk_tx, line bits -> [Vco -> .re -> gain -> RationalResampler ->] Vco (examples/bell202.rs:166-183,
//      g3ruh.rs:256-272).  One push of a.n bits that makes a.na audio samples and a.no outputs (fsk_core.hpp: fsk_plan), all
//      indices relative to the push.  carry_in / carry_out: two device doubles each (phase 1, phase 2), distinct buffers.
//      Scratch, sized by the caller: tilecnt and tiles2 one entry per audio tile of FSK_T; AFSK: audio (the caller's d_audio or
//      scratch) and pre2, na entries; DIRECT: val, na entries.  Launches: the header of kernels_tx.hip.  na == 0 launches nothing.
struct FskTxArgs {
    const unsigned char* bits;
    long n, na, no;
    FskRatio r1, r2;
    long e1, e2;
    long map_dq, map_dr;                      // (FSK_B * D2) / I2 and % I2: what src2 moves by over FSK_B outputs
    double dhi, dlo, k2;                      // k1 * hi, k1 * lo
    float gain;
    const double* carry_in;
    double* carry_out;
    unsigned* tilecnt;
    double* tiles2;
    float* audio;
    double* pre2;
    cf* val;
    cf* out;
};
void launch_fsk_tx(const FskTxArgs& a, bool afsk, hipStream_t s);
// ---- kernels_tx.hip: rr_fsk_tx_multi, the same chain for nstreams streams of one parameter set.  Stream c takes
//      the next min(counts[c], n_cap) bits at bits + c * bits_stride (counts: device, may be null = n_cap each); its push is planned
//      on the device from st_in[c] (fsk_plan) into plan[c], its next state goes to st_out[c] and what it made to made[c] (audio)
//      and made[nstreams + c] (outputs).  Every kernel below the plan is a body of rr_fsk_tx's general path over the view of stream
//      blockIdx.y.  Scratch per stream: tilecnt and tiles2 tpitch = ceil(audio_cap / FSK_T) entries, pre2 / val audio_cap entries;
//      audio is the caller's (audio_stride) or scratch (audio_stride = audio_cap).  Launches: 6 (AFSK) or 5 (DIRECT) whatever the
//      counts and nstreams are; n_cap == 0 launches nothing.
struct FskTxMultiArgs {
    const unsigned char* bits;
    long bits_stride, n_cap, nstreams;
    const unsigned long long* counts;
    FskRatio r1, r2;
    long map_dq, map_dr;
    double dhi, dlo, k2;
    float gain;
    const FskStream* st_in;
    FskStream* st_out;
    FskPush* plan;
    unsigned long long* made;
    long audio_cap, out_cap, tpitch;
    unsigned* tilecnt;
    double* tiles2;
    float* audio;
    long audio_stride;
    double* pre2;
    cf* val;
    cf* out;
    long out_stride;
};
void launch_fsk_tx_multi(const FskTxMultiArgs& m, bool afsk, hipStream_t s);

// ---- kernels_burst.hip: ComplexToMag2, SinglePoleIirFilter and the burst detector as a tiled f64 scan ------------------------
// out[i] = (f32) y_i, y_i = a x_i + b y_(i-1) in f64 fma, y_(-1) = *y_in, i < n; *y_out <- y_(n-1).  y_in and y_out are distinct
// device doubles per row (the block's ping-pong); tiles = device scratch of rows * ceil(n / IIR_T) doubles.  n == 0 launches
// nothing and leaves *y_out alone.
constexpr int IIR_T = 2048;                   // samples of one scan tile
constexpr int IIR_PW8_N = IIR_T / 8 + 1;      // pw8[k] = b^(8 k), k <= IIR_T / 8
constexpr int IIR_SSPAN = 4 * IIR_T;          // samples one thread of k_iir_scan covers
constexpr int IIR_PWS_N = 1024 + 1;           // pws[k] = b^(IIR_SSPAN k), k <= 1024
struct IirCoef {
    double a, b, bT;                          // alpha and fl32(1 - alpha) widened; b^IIR_T
    const double* pw8;                        // device tables of IIR_PW8_N / IIR_PWS_N doubles
    const double* pws;
};
void launch_iir_f32(const float* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles, hipStream_t s);
// Complex: re and im are two rows of the same launches (y_in / y_out: two doubles)
void launch_iir_c32(const cf* in, cf* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles, hipStream_t s);
// x_i = norm_sqr(in[i]) with the reference's three f32 roundings: ComplexToMag2 -> SinglePoleIirFilter on the same scan
void launch_mag2_iir(const cf* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles, hipStream_t s);
// ... and the positions i where (out[i] > thr) differs from (out[i - 1] > thr), out[-1] > thr = *flag_in: entry (i << 1) | cur
// appended at list[atomicAdd(count)], unordered; *flag_out <- out[n - 1] > thr; *count must be 0 on entry, *count_next is zeroed.
// list: n slots.
void launch_burst_detector(const cf* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles,
                           float thr, const int* flag_in, int* flag_out, unsigned long long* count, unsigned long long* count_next,
                           unsigned long long* list, hipStream_t s);
void launch_mag2(const cf* in, float* out, long n, hipStream_t s);    // out[i] = re * re + im * im, three f32 roundings

// ---- kernels_bits.hip: BinarySlicer, XorConst(1), NrziDecode, Descrambler and CorrelateAccessCodeTag as one tile kernel -------
// out[i] = the bit after the last enabled stage, one u8 (0 / 1) per sample, i < n; ONE launch.  st_in / st_out: distinct
// device arrays of BITS_ST_N words (the block's ping-pong): what the stream before the window left, and what this window
// leaves.  With L != 0: for every i whose last L bits differ from the code in <= allowed places once L bits of the stream have
// been seen, an entry (i << 8) | diffs; tile t (BITS_T samples) writes its entries, ascending, to list[t BITS_T ..) and their
// number to tilecnt[t]: ceil(n / BITS_T) counters, as many times BITS_T slots.  No atomics.  n == 0 launches nothing and
// leaves *st_out alone.  launch_bits_tag_offsets / _gather close the gaps: offs[t] = the entries before tile t, *total = all,
// out[0 .. total) = the entries in ascending order.
constexpr int BITS_T = 4096;                  // samples of one tile
enum { BITS_ST_RLAST = 0,                     // r[-1]: the last sliced (and inverted) bit; 0 at the start (nrzi.rs:32-33)
       BITS_ST_DHIST = 1,                     // bit 63 - k = d[-1 - k]: the last 64 bits in front of the descrambler
       BITS_ST_SHIST = 2,                     // bit 63 - k = s[-1 - k]: the last 64 bits in front of the correlator
       BITS_ST_SEEN = 3,                      // bits of the stream so far, saturating at 64
       BITS_ST_N = 4 };
struct BitsCfg {
    int invert, nrzi;                         // XorConst(1); NrziDecode
    unsigned long long dmask;                 // bit (delta - 1) set: s[n] ^= d[n - delta], delta = 1 .. 64; 0 = no descrambler
    unsigned long long code;                  // bit k = code[k], code[0] the oldest
    int L;                                    // code length 1 .. 64; 0 = no correlator
    unsigned allowed;
};
void launch_bits_f32(const float* in, unsigned char* out, long n, const BitsCfg& c, const unsigned long long* st_in,
                     unsigned long long* st_out, unsigned* tilecnt, unsigned long long* list, hipStream_t s);
void launch_bits_u8(const unsigned char* in, unsigned char* out, long n, const BitsCfg& c, const unsigned long long* st_in,
                    unsigned long long* st_out, unsigned* tilecnt, unsigned long long* list, hipStream_t s);
void launch_bits_tag_offsets(const unsigned* tilecnt, long ntiles, unsigned long long* offs, unsigned long long* total, hipStream_t s);
void launch_bits_tag_gather(const unsigned* tilecnt, const unsigned long long* offs, const unsigned long long* list, long ntiles,
                            unsigned long long* out, hipStream_t s);

// ---- kernels_wpcr.hip: Wpcr (wpcr.rs:105-239) over a batch of disjoint bursts of one f32 buffer, four launches ------------------
// Burst b is x[start .. start + n); its scratch lives at the SAME offsets of buffers as long as x: list (the crossing
// positions, tile t's at list[start + t WPCR_T ..)), mag (|X[k]| at mag[start + k], k < (n - 1) / 2), reim (Re X at
// reim[start + k], Im X behind them) and its symbols at syms[start ..).  smap / bmap: the burst of every sample tile (WPCR_T
// samples, ceil(n / WPCR_T) per burst) / bin tile (WPCR_BT bins, ceil(((n - 1) / 2) / WPCR_BT) per burst), tiles in burst order;
// stile0 / btile0: a burst's first tile in them.  tilecnt: one counter per sample tile.  res: one record per burst, laid out as
// rr_wpcr_result.  has_mid == false: mid is 0 in every record and the symbols are the samples' own bits.  nbursts == 0
// launches nothing.
constexpr int WPCR_T = 2048;                  // samples of one tile
constexpr int WPCR_CH = 1024;                 // crossings of one LDS chunk of the transform
constexpr int WPCR_BT = 1024;                 // bins of one tile
struct WpcrBurst {
    long start;
    int n;
    float mid;
    int stile0, btile0;
};
struct WpcrResult {
    int ok;
    unsigned bin;
    float sps, phase0, phase, frequency;
    unsigned long long nsyms;
};
void launch_wpcr(const float* x, const WpcrBurst* bursts, long nbursts, const int* smap, long nstiles, const int* bmap, long nbtiles,
                 bool has_mid, float samp_rate, unsigned* list, unsigned* tilecnt, float* mag, float* reim, WpcrResult* res,
                 float* syms, hipStream_t s);

// ---- kernels_pdu.hip: BurstTagger -> StreamToPdu -> Midpointer over one window of a data / trigger stream pair ------------------
// All positions in the state are ABSOLUTE stream positions; w0 is the window's first.  The arena of a push is the virtual stream
// "open burst ++ window": arena[C + i] = data[i], i < n, and the samples of a burst still open from earlier pushes in front of
// it, ending at arena[C) (C = max_size: an open burst never holds more).  They are taken from the PREVIOUS push's arena
// (prev_arena, whose window was n_prev samples), so the two arenas are the block's double-buffered carry.
// edges: (pos << 1) | cur, ascending, *etotal of them (at most n).  jmp0 / jmp1 / mark: n / 2 + 2 entries each.  recs: n / 2 + 2
// records, appended in no order; *count of them (zeroed by the launcher).  n == 0 launches nothing.
constexpr int PDU_T = 2048;                   // samples of one tile
constexpr unsigned long long PDU_NONE = ~0ull;
struct PduState {
    unsigned long long free;                  // the first position at which a rising edge is taken again
    unsigned long long open_r, open_f;        // the accepted burst that has not been filed yet: its rising edge and, once seen, its
                                              // falling edge (PDU_NONE otherwise)
    int last, pad;                            // cur(-1)
};
struct PduRoot {                              // what the carried state and the window's first edge decide (k_pdu_next)
    unsigned long long free;                  // `free` in front of the window's first rising edge
    unsigned long long open_r, open_f;        // the carried burst after the window's first edge has been seen
    long j0;                                  // the first accepted rising edge of the window (R: none)
    long R;                                   // rising edges of the window
};
struct PduRec {                               // rr_pdu_record
    unsigned long long start, len, stream_pos;
    int ok;
    float mean, mid;
    unsigned long long nlow;
};
enum { PDU_F32 = 0, PDU_C32 = 1, PDU_NODATA = 2 };   // the element of data / arena / prev_arena; NODATA: the caller fills the arena
struct PduArgs {
    const void* data;
    const float* trig;
    long n;
    float thr;
    unsigned long long max_size, tail, w0;
    long C;
    const void* prev_arena;
    long n_prev;
    void* arena;
    const PduState* st_in;
    PduState* st_out;
    unsigned* tilecnt;
    unsigned long long* offs;
    unsigned long long* etotal;
    unsigned* edges;
    unsigned* jmp0;
    unsigned* jmp1;
    unsigned* mark;
    PduRoot* root;
    PduRec* recs;
    long rec_cap;
    unsigned long long* count;
    float* ranks;                             // with midpoint: low and high of record slot k at [2 k], [2 k + 1] (0 when ok == 0)
    bool midpoint;
};
void launch_pdu(const PduArgs& a, hipStream_t s, int elem = PDU_F32);

// ---- kernels_saver.hip: Delay, and Delay -> the arena of StreamToPdu<Complex> (examples/burst_saver.rs) ------------------------------
// out[i] = 0 (all zero bytes) for i < zeros, in[i - zeros] for the `copied` elements behind them; es = 1, 4 or 8 bytes, pointers
// aligned to es.  One launch; nothing to write launches nothing.
void launch_delay(const void* in, void* out, long zeros, long copied, size_t es, hipStream_t s);
// One window of the burst saver's data branch, Complex samples as 64-bit words: arena[C + i] = the delayed window (i < from_hist:
// hist_in[i], else x[i - delay]), the open burst of the previous arena in front of arena[C) exactly as k_pdu_tiles places it, and
// hist_out = the last `delay` input samples (j < shifted: hist_in[j + n], else x[j + n - delay]).  from_hist / shifted:
// saver_host.hpp saver_plan.  hist_in and hist_out are distinct.  One launch; n == 0 launches nothing.
struct SaverArgs {
    const unsigned long long* x;
    long n, delay, from_hist, shifted;
    const unsigned long long* hist_in;
    unsigned long long* hist_out;
    unsigned long long* arena;
    long C;
    const unsigned long long* prev_arena;
    long n_prev;
    const PduState* st_in;
    unsigned long long w0;
};
void launch_saver_copy(const SaverArgs& a, hipStream_t s);
// PduToStream over a batch: out[dst[b] + i] = syms[src[b] + i], i < len[b]; desc holds nb (src, dst, len) triples ascending in
// dst without gaps, total = their lengths' sum.  One launch; total == 0 launches nothing.
void launch_pdu_pack(const float* syms, const long* desc, long nb, long total, float* out, hipStream_t s);

// ---- kernels_frame.hip: FcsAdder -> HdlcFramer -> PduToStream<u8> over a batch of packets, then Scrambler::g3ruh -> NrziEncode ->
//      Map over the stream they make (frame_core.hpp holds the arithmetic) -----------------------------------------------------------
// Packet p is bytes[starts[p] ..) followed by its two FCS bytes when fcs != 0; pb[p] = the bytes of the packets before it with
// their FCS bytes (pb[P] = nbytes), cpre[p] = the CRC chunks (FRAME_CH payload bytes each) before it.  The payload bits of all
// packets, back to back, are cut into tiles of FRAME_T bits: ntiles = max(1, ceil(8 nbytes / FRAME_T)).  pre gets the framed
// bits, one u8 each; cb[b], b <= P: the stuffed bits before packet b's first payload bit; *total: the framed bits of the push.
// Scratch: part (cpre[P] words), crc (P), lb (nbytes), sums (ntiles StuffSums = 4 words each), tin (2 ntiles).  P == 0 launches
// nothing.  The launches depend on P, nbytes and fcs alone.
constexpr int FRAME_T = 4096;                 // payload bits of one tile
constexpr int FRAME_CH = 128;                 // payload bytes of one CRC chunk
struct FrameArgs {
    const unsigned char* bytes;
    const unsigned long long* starts;
    const unsigned long long* pb;
    const unsigned long long* cpre;
    long P, nbytes, ntiles, nchunks;          // nchunks = cpre[P]
    int fcs;
    unsigned* part;
    unsigned* crc;
    unsigned char* lb;
    unsigned* sums;
    unsigned* tin;
    unsigned* cb;
    unsigned long long* total;
    unsigned char* pre;
    long cap;                                 // elements of pre: the bound of the push
};
void launch_frame(const FrameArgs& a, hipStream_t s);
// The line coder over n bits, u8 in (the lowest bit of each): out = u8 bits, or with out_f32 bit ? hi : lo.  n = *n_dev when
// n_dev is given (then at most max_n, which sizes the grid and the scratch), else max_n.  mode: LINE_SCR | LINE_NRZI
// (frame_core.hpp); pw: the LINE_NP powers of the tile matrix for that mode.  st_in / st_out: distinct device words (the
// block's ping-pong), the state in front of the window and behind it.  z, carry: ceil(max_n / LINE_T) words each.  Three
// launches, or one when mode == 0 (then no state is read or written); max_n == 0 launches nothing.
struct LineArgs {
    const unsigned char* in;
    void* out;
    int out_f32;
    float lo, hi;
    long max_n;
    const unsigned long long* n_dev;
    int mode;
    const unsigned* pw;
    const unsigned* st_in;
    unsigned* st_out;
    unsigned* z;
    unsigned* carry;
};
void launch_line(const LineArgs& a, hipStream_t s);

// ---- kernels_kiss.hip: KissFrame -> KissDecode (kiss.rs:96-228) over the next n bytes of a stream, and KissEncode -> PduToStream
//      (kiss.rs:247-286) over a batch of packets (kiss_core.hpp holds the arithmetic) ----------------------------------------------------
// The VIRTUAL stream of a decode push: the st_in->carry bytes of the gap still open (cin), then bytes[0 .. n).  nv_max >= carry + n
// is the host's own bound; it alone sizes the grids and the scratch: ntiles = ceil(nv_max / KISS_T) entries of sums / tin / tsum /
// toff (tsum: 5 words a tile), ntiles + 1 of obase (all ones on entry).  Packets go to arena packed in stream order, their records
// to recs in the same order, *count of them and *total bytes.  st_out / cout: what the next push starts from (distinct from st_in /
// cin).  KISS_DECODE_LAUNCHES launches whatever the bytes hold; n == 0 launches nothing.
constexpr int KISS_DECODE_LAUNCHES = 6, KISS_ENCODE_LAUNCHES = 3;
struct KissState {
    unsigned long long stats[5];              // frames, delivered, nondata, bad_escape, overlong so far
    int code;                                 // KISS_VIRT / KISS_UNSYNC / KISS_OVER
    unsigned carry;                           // carried bytes (KISS_VIRT only)
};
struct KissRec {                              // rr_kiss_packet
    unsigned long long pos, start;
    unsigned len, in_bytes, port, reserved;
};
struct KissArgs {
    const unsigned char* bytes;
    long n;
    const unsigned char* cin;
    unsigned char* cout;
    const KissState* st_in;
    KissState* st_out;
    unsigned max_len;                         // bytes of cin / cout
    long nv_max, ntiles;
    unsigned long long w0;                    // stream position of bytes[0]
    unsigned* sums;                           // 6 words a tile: its KissSum
    unsigned* tin;                            // ... and the summary of everything in front of it
    unsigned* root;                           // the summary of the whole virtual stream
    unsigned* tsum;                           // packets, bytes, nondata, bad escapes, over-long gaps closed in the tile
    unsigned* toff;                           // 2 words a tile: the packets and bytes in front of it
    unsigned* obase;                          // where the gap opened by a tile's last FEND (slot tile + 1; 0: the carried one) goes
    unsigned char* arena;
    long arena_cap;
    KissRec* recs;
    long rec_cap;
    unsigned long long* count;                // [0] packets, [1] arena bytes
};
void launch_kiss_decode(const KissArgs& a, hipStream_t s);
// Packet p is bytes[starts[p] ..), pb[p] the bytes of the packets before it (pb[P] = nbytes), ports[p] its port.  The packets' bytes,
// back to back, are cut into tiles of KISS_T: ntiles = max(1, ceil(nbytes / KISS_T)) entries of tcnt / tin.  cb[b], b <= P: the escaped
// bytes in front of packet b; *total: the bytes of the push.  KISS_ENCODE_LAUNCHES launches whatever the packets hold; P == 0 none.
struct KissEncArgs {
    const unsigned char* bytes;
    const unsigned long long* starts;
    const unsigned long long* pb;
    const unsigned long long* ports;
    long P, nbytes, ntiles;
    unsigned* tcnt;
    unsigned* tin;
    unsigned* cb;
    unsigned long long* total;
    unsigned char* out;
    long cap;                                 // bytes of out: the bound of the push
};
void launch_kiss_encode(const KissEncArgs& a, hipStream_t s);

// ---- kernels_hdlc.hip: HdlcDeframer (hdlc_deframer.rs:123-232) over the next n bits of a stream (hdlc_core.hpp holds the
//      arithmetic) -------------------------------------------------------------------------------------------------------------------------
// The VIRTUAL stream of a push: the st_in->count bits the stream so far left in cin (HDLC_HALO bits, then the raw bits of the gap
// still open), then bits[0 .. n).  nv_max >= count + n is the host's own bound; it alone sizes the grids and the scratch, and
// hdlc_plan (hdlc_host.hpp) is the one place that says how: the words of raw / fl / ab / sf, the tiles of tilecnt / offs, ends_cap
// flag ends and gap maps, the block maps and states (HDLC_T and HDLC_GB: hdlc_dims.hpp).  Frames go to arena (arena_cap bytes,
// zeroed by the caller) at byte floor((s + 1) / 8) of the gap's first flag end s, their records to recs in no order, *count of
// them; pstats: this push's share of the three counters.  st_out / cout: what the next push starts from (distinct from st_in /
// cin).  Seven launches whatever the bits hold; n == 0 launches nothing.
struct HdlcState {
    unsigned long long stats[3];              // decoded, crc_error, bitfixed so far
    unsigned count;                           // carried bits
    int state;                                // the machine at the anchor, carried bit HDLC_HALO - 1
};
struct HdlcRec {                              // rr_hdlc_frame
    unsigned long long pos, start;
    unsigned len, flags;
};
struct HdlcArgs {
    const unsigned char* bits;
    long n;
    const unsigned char* cin;
    unsigned char* cout;
    const HdlcState* st_in;
    HdlcState* st_out;
    long carry_cap;                           // bytes of cout
    long nv_max, ntiles;
    unsigned long long w0;                    // stream position of bits[0]
    unsigned long long min_size, max_size;
    int keep, fix;
    unsigned long long *raw, *fl, *ab, *sf;
    unsigned* tilecnt;
    unsigned long long* offs;
    unsigned long long* etotal;
    unsigned* ends;
    long ends_cap;
    unsigned char *gmap, *pmap, *bmap, *bstate;
    int* fin;
    unsigned char* arena;
    long arena_cap;
    HdlcRec* recs;
    long rec_cap;
    unsigned long long* count;
    unsigned long long* pstats;
};
void launch_hdlc(const HdlcArgs& a, hipStream_t s);

// ---- kernels_hdlcrx.hip: BinarySlicer -> [XorConst(1)] -> [NrziDecode] -> [Descrambler] -> HdlcDeframer over the next symbols of
//      nstreams independent streams (hdlcrx_core.hpp holds the bit chain in word form, hdlc_body.hpp the deframer's kernels) -----
// Stream c: min(counts ? counts[c] : n_cap, n_cap) f32 symbols at syms + c stride, read on the device; nothing at or beyond
// that count is read.  `h` is stream 0's view with the HOST's bounds in nv_max / ntiles / ends_cap / arena_cap (one number serves
// all streams) and a null `bits`; stream c's buffers stand c pitches further on, which are hdlc_plan's numbers: p_words words of
// raw / fl / ab / sf, p_tiles of tilecnt / offs, p_ends of ends / gmap / pmap, p_blocks of bmap / bstate, p_carry bytes of cin /
// cout, p_arena bytes of arena, one etotal / fin / st_in / st_out and three pstats each.  bst_in / bst_out: RX_ST_N words per
// stream (hdlcrx_core.hpp).
// h.count is ONE counter and recs ONE list of rec_cap records for all streams; a record's start is absolute (c p_arena + ...).
// The seven launches of launch_hdlc with the stream as the grid's y, whatever nstreams and the symbols are; n_cap == 0 launches
// nothing.  A stream with no symbols has its state copied from the in to the out buffers.
struct HdlcRxRec {                            // rr_hdlc_stream_frame
    unsigned long long pos, start;
    unsigned len, flags, stream, reserved;
};
struct HdlcRxArgs {
    const float* syms;
    long stride, n_cap, nstreams;
    const unsigned long long* counts;         // may be null: every stream has n_cap
    int invert, nrzi;
    unsigned long long dmask;                 // BitsCfg::dmask
    const unsigned long long* bst_in;
    unsigned long long* bst_out;
    HdlcArgs h;
    long p_words, p_tiles, p_ends, p_blocks, p_carry, p_arena;
    HdlcRxRec* recs;
};
void launch_hdlcrx(const HdlcRxArgs& a, hipStream_t s);

// ---- kernels_il2p.hip: BinarySlicer -> [XorConst(1)] -> CorrelateAccessCodeTag(il2p SYNC_WORD) -> Il2pDeframer over the next
//      symbols of nstreams independent streams (il2p_core.hpp holds the arithmetic) --------------------------------------
// Stream c: min(counts ? counts[c] : n_cap, n_cap) f32 symbols at syms + c stride, read on the device; nothing at or beyond that
// count is read.  Its state goes from st_in to st_out (IL2P_ST_N words each, distinct).  Scratch, all sized by the HOST's bound
// ntiles = ceil(n_cap / IL2P_T): bits holds p_words = IL2P_CARRY_WORDS + 64 ntiles + 1 words of its virtual stream, mw 64 ntiles
// match words, maps IL2P_MAP_PITCH bytes per tile, entry one byte per tile.  recs is ONE list of rec_cap records and *count ONE
// counter for all streams (zeroed by the caller); stats: headers, syncs per stream, added to.  Three launches whatever nstreams,
// the counts and the symbols are; n_cap == 0 launches nothing.
struct Il2pArgs {
    const float* syms;
    long stride, n_cap, nstreams;
    const unsigned long long* counts;         // may be null: every stream has n_cap
    int invert;
    unsigned allowed;                         // allowed_diffs, clamped to 24
    const unsigned long long* st_in;
    unsigned long long* st_out;
    unsigned long long *bits, *mw;
    long p_words, ntiles;
    unsigned char *maps, *entry;
    Il2pRec* recs;
    long rec_cap;
    unsigned long long* count;
    unsigned long long* stats;
};
void launch_il2p(const Il2pArgs& a, hipStream_t s);

// ---- kernels_sync.hip: SymbolSync (symbol_sync.rs:115-217) over the next n samples of nstreams independent streams
//      (symsync_core.hpp holds the arithmetic) -------------------------------------------------------------------------------------------
// Stream c: n samples at in + c in_stride; its symbols at syms + c out_stride, its clock values (clk may be null) at
// clk + c out_stride, count[c] of each; its state from st_in[c] to st_out[c] (distinct).  Scratch: words[c nwords + w] holds
// the signs of samples 64 w .. 64 w + 63 of stream c (nwords = ceil(n / 64)), idx[c n + k] the window-relative index of
// emission k.  Three launches whatever the samples hold (launch_sync: signs, clock, gather); which = 1 .. 3 runs that one alone.
// spw: streams per wave of the clock kernel, 1 (one active lane per wave) or 64.
struct SyncArgs {
    const float* in;
    long in_stride, n, nstreams;
    float* syms;
    float* clk;
    long out_stride;
    unsigned long long* words;
    long nwords;
    unsigned* idx;
    unsigned long long* count;
    const SyncState* st_in;
    SyncState* st_out;
    SyncParams prm;
    int spw;
};
void launch_sync(const SyncArgs& a, int which, hipStream_t s);

// ---- kernels_afsk.hip: Hilbert -> QuadratureDemod -> FftFilterFloat (direct form) -> AddConst over the next a.n samples of
//      nstreams independent streams (afsk_core.hpp holds AfskArgs, the arithmetic and the indexing).  ONE launch whatever nstreams
//      and n are (none for n == 0): grid (tiles of AFSK_TILE outputs, at least one; nstreams).  a.carry_in and a.carry_out are
//      distinct; a.taps and a.hr are device pointers.
void launch_afsk(const AfskArgs& a, long nstreams, hipStream_t s);

// ---- kernels_am.hip: norm -> FftFilterFloat (direct form, only the outputs the resampler picks) -> RationalResampler ->
//      MultiplyConst over the next a.n Complex samples of nstreams independent streams (am_core.hpp holds AmArgs, the arithmetic
//      and the indexing).  ONE launch whatever nstreams, n, the taps and the ratio are (none for n == 0): grid (tiles of a.g.T
//      outputs, at least one; nstreams), am_lds_bytes() of LDS.  a.carry_in and a.carry_out are distinct; a.taps is a device pointer.
size_t am_lds_bytes();
void launch_am(const AmArgs& a, long nstreams, hipStream_t s);
// AirSPY u32 samples (i16 I low, i16 Q high) -> Complex(i / 1000, q / 1000), true f32 divisions
void launch_airspy_decode(const unsigned* in, cf* out, long n, hipStream_t s);

// ---- kernels_pwm.hip: [ComplexToMag2 ->] PwmDecoder (pwm_decoder.rs:385-513) over the next n samples of a stream (pwm_core.hpp
//      holds the arithmetic) -----------------------------------------------------------------------------------------------------------
// in: n f32 power samples (es 4) or n Complex samples (es 8: norm_sqr with the reference's three roundings in front).  Scratch,
// all sized from n by pwm_plan (pwm_host.hpp): cls / ebits one word / byte per thread of every tile, tmap / tstate / tilecnt /
// offs one per tile, edges ecap >= n entries.  The carried halves (st, fbits, meta, cand: in and out distinct) hold the slicer
// state, the open frame and the candidate table, `pitch` bytes per candidate row.  Deliveries: recs in delivery order, their bits
// in arena at rec.start; count[0] = records, count[1] = arena bytes, both counted on past the capacities (the host refuses such a
// push).  Seven launches whatever the samples hold; n == 0 launches nothing.  eof: no samples — the candidates are delivered
// (two launches).
struct PwmArgs {
    const void* in;
    int es, eof;
    long n, ntiles, ecap;
    PwmCfg cfg;
    unsigned long long pitch;
    const PwmState* st_in;
    PwmState* st_out;
    const unsigned char* fbits_in;
    unsigned char* fbits_out;
    const PwmCand* meta_in;
    PwmCand* meta_out;
    const unsigned char* cand_in;
    unsigned char* cand_out;
    unsigned short* cls;
    unsigned char *tmap, *tstate, *ebits;
    unsigned *tilecnt, *offs, *edges;
    unsigned long long* etotal;
    PwmRec* recs;
    long rec_cap;
    unsigned char* arena;
    long arena_cap;
    unsigned long long* count;
};
constexpr int PWM_LAUNCHES = 7;
void launch_pwm(const PwmArgs& a, hipStream_t s);

// ---- head fix of the fused FirFilter -> FftFilter blocks (stream start only, a few hundred samples) ----------------
// z[m] = sum_k t1[k] V[voff + m + L1 - 1 - k], m < n: the front FirFilter's first outputs (fir.rs:166-177) from the virtual stream
void launch_head_z(VSrc<cf> V, long voff, const cf* t1, int L1, cf* z, long n, hipStream_t s);
// y[i] = sum_{j <= min(i, L2 - 1)} t2[j] z[i - j], i < n: FftFilter's zero-history head (fft_filter.rs:332-348)
void launch_head_y(const cf* z, const cf* t2, int L2, cf* y, long n, hipStream_t s);
// the same head resampled (r[u] = y[floor(u D / I)]) and demodulated: rewrites out[u - 1] for every u < r_hi whose pair
// touches y[n], n < L2 - 1, and *last_r when r[r_hi - 1] does (nz = valid entries of z)
void launch_head_demod(const cf* z, long nz, const cf* t2, int L2, long I, long D, float gain, int mode, long r_hi, float* out,
                       cf* last_r, hipStream_t s);

// ---- glue of the any-size transforms (kernels_misc.hip; see AnyFft in blocks.hpp) --------------------------------------
void launch_transpose_tw(const cf* in, cf* out, int rows, int cols, long nframes, const cf* tw, hipStream_t s);
void launch_chirp_pre(const cf* in, cf* a, long N, long M, long nframes, const cf* chirp, hipStream_t s);
void launch_mul_conj(cf* a, const cf* b, long M, long nframes, hipStream_t s);
void launch_chirp_post(const cf* y, cf* out, long N, long M, long nframes, const cf* chirp, hipStream_t s);
void launch_ols_gather(VSrc<cf> src, cf* frames, long S, long M, long f0, long nframes, hipStream_t s);
void launch_ols_scatter(const cf* frames, cf* out, long S, long M, long L, long f0, long nframes, long n_out, hipStream_t s);

int device_cu_count();

}  // namespace rr
