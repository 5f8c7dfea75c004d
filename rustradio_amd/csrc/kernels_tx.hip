// kernels_tx.hip — Vco (src/vco.rs:9-37) and the fused RationalResampler -> Vco of examples/fm_tx.rs:84-91.
//
// The reference's phase is a running f64 sum: phase += k * a, one wrap by MX = 2 pi when it leaves [-MX, MX], then
// (sin, cos).  Only sin(phase) and cos(phase) are observable, so any representative of the phase modulo MX serves, and the
// sum becomes a scan in three launches ordered by the stream alone:
//   k_vco_sums    per tile of VCO_T samples the sum of its k * a, folded into [-MX, MX]
//   k_vco_scan    ONE workgroup: exclusive scan of the tile sums on top of the phase carried in from the previous call
//                 (device memory, ping-pong), in place; writes the phase carried out
//   k_vco_apply   per tile the inclusive scan of its samples from the tile's base, f64 sincos, one 8-byte store per sample
// A window of one tile runs k_vco_apply alone, with the carried phase as its base.
// No workgroup waits on another one: no look-back, no ticket, no spinning on a flag.
//
// Every addition of the scan is followed by the reference's own wrap, so no intermediate leaves [-2 MX, 2 MX] and one
// addition costs at most half an ulp of 4 pi, as in the sequential form (DESIGN.md "Vco").  A non-finite sample makes its
// own prefix sum and every later one NaN or +-Inf, whose sin and cos are NaN: the reference's behaviour with no pass for it.
// Exclusive prefixes are built from the earlier elements only (never inclusive minus own), so the samples before stay clean.
//
// rr_fsk_tx (examples/bell202.rs:166-183, g3ruh.rs:256-272): both VCOs of the packet transmitters with every scan
// at the AUDIO rate.  Stage 1 has two levels, so its phase at audio sample m is k1 hi c1 + k1 lo c0 with c1 / c0 the one- and
// zero-samples up to m: an integer scan, and the phase is formed from the counts directly (fsk_phase1), no f64 sum at all.
// Stage 2's input is constant over the rep2(m) outputs of an audio sample, so its f64 scan runs over rep2(m) * (k2 a[m]) per
// audio sample and the output-rate kernel is a map.  Launches of a push (na audio samples, no outputs; never a matter of the bits):
//                                      AFSK                                          DIRECT
//   na == 0                            0                                             0
//   na <= FSK_T (one audio tile)       2: k_fsk_audio, k_fsk_map                     2: k_fsk_audio, k_fsk_map
//   na >  FSK_T                        5: k_fsk_count, k_fsk_scan1, k_fsk_audio,     4: k_fsk_count, k_fsk_scan1, k_fsk_audio,
//                                         k_vco_scan, k_fsk_map                         k_fsk_map
// and one fewer where no == 0 (every audio sample of the push is one the second resampler drops: k_fsk_map has nothing to do).
// As above, no workgroup waits on another one and there is no atomic.
//
// rr_fsk_tx_multi: the same chain for nstreams streams of one parameter set, the counts of a push read on the
// device.  k_fskm_plan plans every stream's push from the FskPos it carries; the five kernels of the na > FSK_T column run as
// k_fskm_* over the view of stream blockIdx.y (the bodies are shared with the kernels above), always, since the host does not
// know the counts: 6 launches in AFSK mode, 5 in DIRECT, whatever the counts, the bits and nstreams are; none for n_cap == 0.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

constexpr int VCO_B = 256;                    // threads of a workgroup
constexpr int VCO_PER = VCO_T / VCO_B;        // consecutive samples of one thread
static_assert(VCO_PER == 8 && VCO_B == 256, "k_vco_apply: 8 samples per thread");
constexpr double VCO_MX = 2.0 * 3.14159265358979323846;   // vco.rs: 2.0 * f64::consts::PI

// vco.rs:27-32, both tests in the reference's order.  |p| <= 2 MX in, |p| <= MX out; v - MX is exact there (Sterbenz).
// NaN passes both comparisons untouched and Inf - MX = Inf.
__device__ __forceinline__ double vco_wrap(double p) {
    if (p > VCO_MX) p -= VCO_MX;
    if (p < -VCO_MX) p += VCO_MX;
    return p;
}
// one sample's increment k * a into [-MX, MX]: beyond 2 MX by whole turns first (the reference lets such a phase grow instead)
__device__ __forceinline__ double vco_step(double k, float a) {
    double d = k * (double)a;
    if (fabs(d) > 2.0 * VCO_MX) d = fma(-VCO_MX, trunc(d * (1.0 / VCO_MX)), d);
    return vco_wrap(d);
}

// sin and cos of a wrapped phase.  |p| <= MX always holds for finite input, so the argument reduction is one rounding to
// the nearest quarter turn and a two-part pi/2 (exact in the FMA), and what is left on [-pi/4, pi/4] takes the two fdlibm
// minimax kernels (k_sin.c / k_cos.c, Sun Microsystems 1993, freely usable): under 1.2e-16 absolute against long double
// over [-MX, MX] (checked on the CPU), an eighth of one sample's share of the error bound.  It saves the library routine's
// general reduction; measured, that is a few per cent of k_vco_apply (profiles/fm_tx_probe.md).  Anything else — NaN, +-Inf,
// a phase a huge k * a left outside — takes the library's.
__device__ __forceinline__ void vco_sincos(double p, double* sn, double* cs) {
    if (!(fabs(p) <= VCO_MX)) { sincos(p, sn, cs); return; }
    const double n = rint(p * 6.36619772367581382433e-01);                        // 2 / pi
    double r = fma(-n, 1.57079632679489655800e+00, p);                            // pi / 2, high part
    r = fma(-n, 6.12323399573676603587e-17, r);                                   // ... and what f64 left of it
    const double z = r * r;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double sr = r + r * z * ps;
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double cr = w + (((1.0 - w) - hz) + z * z * pc);
    const int q = (int)n & 3;                 // sin(r + q pi/2), cos(r + q pi/2)
    const double a = (q & 1) ? cr : sr, b = (q & 1) ? sr : cr;
    *sn = (q & 2) ? -a : a;
    *cs = ((q + 1) & 2) ? -b : b;
}

// The sample behind output o.  FUSED: the resampler's closed-form index map of k_resample (kernels_misc.hip) — the first r
// outputs repeat the pending sample, output r + m reads in[floor((m D - c0) / I)].
template <bool FUSED> struct VcoSrc {
    const float* in;
    const float* pending;
    long r, I, D, c0;
    __device__ __forceinline__ float load(long o) const {
        if (!FUSED) return in[o];
        if (o < r) return pending[0];
        const long m = o - r;
        return in[(I == 1) ? (m * D - c0) : (m * D - c0) / I];
    }
};

// Exclusive scan of one value per thread over a workgroup of NW waves (wrapped sums); total = the sum of all.  s_w: NW doubles.
template <int NW> __device__ __forceinline__ double vco_block_scan(double v, double* s_w, double& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double u = __shfl_up(inc, off, 64);
        if (lane >= off) inc = vco_wrap(u + inc);
    }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    double woff = 0.0, tot = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const double t = s_w[j];
        if (j < w) woff = vco_wrap(woff + t);
        tot = vco_wrap(tot + t);
    }
    __syncthreads();                          // s_w is free again
    total = tot;
    return vco_wrap(woff + exc);
}

template <bool FUSED>
__global__ __launch_bounds__(VCO_B) void k_vco_sums(VcoSrc<FUSED> src, long n, double k, double* __restrict__ tiles) {
    __shared__ double s_w[VCO_B / 64];
    const long ntiles = (n + VCO_T - 1) / VCO_T;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long o0 = tile * VCO_T;
        const int cnt = (int)(n - o0 < VCO_T ? n - o0 : VCO_T);
        double run = 0.0;
        for (int j = threadIdx.x; j < cnt; j += VCO_B) run = vco_wrap(run + vco_step(k, src.load(o0 + j)));
        double total;
        (void)vco_block_scan<VCO_B / 64>(run, s_w, total);
        if (threadIdx.x == 0) tiles[tile] = total;
    }
}

// tiles[i] <- carried phase + tiles[0] + ... + tiles[i - 1]; *carry_out <- carried phase + all of them.  One workgroup of
// VCO_SB threads walks the tile sums in chunks of VCO_SB * 4 through LDS (coalesced both ways; 1e8 samples are 12 chunks).
constexpr int VCO_SB = 1024, VCO_SPER = 4, VCO_SCHUNK = VCO_SB * VCO_SPER;
__device__ __forceinline__ void vco_scan_body(double* __restrict__ tiles, long ntiles, const double* __restrict__ carry_in,
                                              double* __restrict__ carry_out) {
    __shared__ double s_t[VCO_SCHUNK];
    __shared__ double s_w[VCO_SB / 64];
    double base = carry_in[0];
    for (long c0 = 0; c0 < ntiles; c0 += VCO_SCHUNK) {
        const int cnt = (int)(ntiles - c0 < VCO_SCHUNK ? ntiles - c0 : VCO_SCHUNK);
        for (int j = threadIdx.x; j < VCO_SCHUNK; j += VCO_SB) s_t[j] = j < cnt ? tiles[c0 + j] : 0.0;
        __syncthreads();
        double* mine = s_t + threadIdx.x * VCO_SPER;
        double e[VCO_SPER], run = 0.0;
#pragma unroll
        for (int i = 0; i < VCO_SPER; ++i) { e[i] = run; run = vco_wrap(run + mine[i]); }   // exclusive: earlier tiles only
        double total;
        const double exc = vco_block_scan<VCO_SB / 64>(run, s_w, total);
        const double p0 = vco_wrap(base + exc);
#pragma unroll
        for (int i = 0; i < VCO_SPER; ++i) mine[i] = vco_wrap(p0 + e[i]);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += VCO_SB) tiles[c0 + j] = s_t[j];
        base = vco_wrap(base + total);
        __syncthreads();                      // the next chunk overwrites s_t
    }
    if (threadIdx.x == 0) carry_out[0] = base;
}
__global__ __launch_bounds__(VCO_SB) void k_vco_scan(double* __restrict__ tiles, long ntiles, const double* __restrict__ carry_in,
                                                     double* __restrict__ carry_out) {
    vco_scan_body(tiles, ntiles, carry_in, carry_out);
}

// SINGLE: the window is one tile — base[0] is the carried phase and the kernel writes the phase carried out itself.
template <bool FUSED, bool SINGLE>
__global__ __launch_bounds__(VCO_B) void k_vco_apply(VcoSrc<FUSED> src, cf* __restrict__ out, long n, double k,
                                                     const double* __restrict__ base, double* __restrict__ carry_out) {
    // the tile's samples, then its outputs, so that both are coalesced in HBM whatever the window's alignment; one pad per
    // thread (8 elements) keeps the threads' own runs on different LDS banks
    __shared__ cf s_buf[VCO_T + VCO_B];
    __shared__ double s_w[VCO_B / 64];
    float* s_a = reinterpret_cast<float*>(s_buf);
    cf* s_o = s_buf;
    const long ntiles = (n + VCO_T - 1) / VCO_T;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long o0 = tile * VCO_T;
        const int cnt = (int)(n - o0 < VCO_T ? n - o0 : VCO_T);
        for (int j = threadIdx.x; j < VCO_T; j += VCO_B) s_a[j + j / VCO_PER] = j < cnt ? src.load(o0 + j) : 0.0f;
        __syncthreads();
        const int i0 = threadIdx.x * VCO_PER, l0 = threadIdx.x * (VCO_PER + 1);
        double d[VCO_PER];
        double run = 0.0;
#pragma unroll
        for (int i = 0; i < VCO_PER; ++i) {   // inclusive sums from the thread's first sample
            if (i0 + i < cnt) run = vco_wrap(run + vco_step(k, s_a[l0 + i]));
            d[i] = run;
        }
        double total;
        const double exc = vco_block_scan<VCO_B / 64>(run, s_w, total);   // (its barriers: every thread has read s_a before s_o is written)
        const double b = base[SINGLE ? 0 : tile];
        const double p0 = vco_wrap(b + exc);
#pragma unroll
        for (int i = 0; i < VCO_PER; ++i) {
            double sn, cs;
            vco_sincos(vco_wrap(p0 + d[i]), &sn, &cs);
            s_o[l0 + i] = mkcf((float)sn, (float)cs);          // vco.rs:33-36: re = sin, im = cos
        }
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += VCO_B) out[o0 + j] = s_o[j + j / VCO_PER];
        if (SINGLE && threadIdx.x == 0) carry_out[0] = vco_wrap(b + total);
        __syncthreads();                      // the next tile overwrites s_buf
    }
}

template <bool FUSED>
static void vco_launch(VcoSrc<FUSED> src, cf* out, long n, double k, const double* carry_in, double* carry_out, double* tiles,
                       hipStream_t s) {
    if (n <= 0) return;
    const long ntiles = (n + VCO_T - 1) / VCO_T;
    if (ntiles == 1) {
        hipLaunchKernelGGL((k_vco_apply<FUSED, true>), dim3(1), dim3(VCO_B), 0, s, src, out, n, k, carry_in, carry_out);
        RR_HIP(hipGetLastError());
        return;
    }
    const unsigned g = tiles_grid(ntiles);
    hipLaunchKernelGGL((k_vco_sums<FUSED>), dim3(g), dim3(VCO_B), 0, s, src, n, k, tiles);
    hipLaunchKernelGGL(k_vco_scan, dim3(1), dim3(VCO_SB), 0, s, tiles, ntiles, carry_in, carry_out);
    hipLaunchKernelGGL((k_vco_apply<FUSED, false>), dim3(g), dim3(VCO_B), 0, s, src, out, n, k, (const double*)tiles, carry_out);
    RR_HIP(hipGetLastError());
}

void launch_vco(const float* in, cf* out, long n, double k, const double* carry_in, double* carry_out, double* tiles, hipStream_t s) {
    vco_launch(VcoSrc<false>{in, nullptr, 0, 1, 1, 0}, out, n, k, carry_in, carry_out, tiles, s);
}
void launch_fm_tx(const float* in, cf* out, long r, const float* pending, long n_gather, long I, long D, long c0, double k,
                  const double* carry_in, double* carry_out, double* tiles, hipStream_t s) {
    vco_launch(VcoSrc<true>{in, pending, r, I, D, c0}, out, r + n_gather, k, carry_in, carry_out, tiles, s);
}

// ---- rr_fsk_tx (see the header comment; fsk_core.hpp has the index maps and the phase arithmetic) ---------------------------------
static_assert(FSK_T == FSK_B * FSK_PER && FSK_OT == FSK_B * FSK_PER && FSK_B == VCO_B, "8 audio samples / 8 outputs per thread");
static_assert(FSK_MX == VCO_MX && FSK_SCAN_CHUNK == VCO_SCHUNK, "one 2 pi, one scan chunk");

// Exclusive scan of one count per thread over a workgroup of NW waves; total = the sum of all.  s_w: NW unsigneds.
template <int NW> __device__ __forceinline__ unsigned fsk_block_scan(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned woff = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const unsigned t = s_w[j];
        if (j < w) woff += t;
        tot += t;
    }
    __syncthreads();                          // s_w is free again
    total = tot;
    return woff + inc - v;
}

// bit j of the result: audio sample m0 + j of the push is a one-sample (its bit is nonzero: the reference's s > 0), j < cnt <= 8
__device__ __forceinline__ unsigned fsk_ones8(const FskTxArgs& a, long m0, int cnt) {
    unsigned mask = 0;
    if (cnt <= 0) return 0;
    FskWalk w = fsk_walk_src(a.r1, a.e1, m0);
#pragma unroll
    for (int j = 0; j < FSK_PER; ++j) {
        if (j < cnt) {
            mask |= (a.bits[w.q] != 0 ? 1u : 0u) << j;
            w.next();
        }
    }
    return mask;
}

// The kernels' bodies are device functions over one stream's FskTxArgs: rr_fsk_tx's kernels pass their own argument, rr_fsk_tx_multi's
// the view of stream blockIdx.y (fskm_view below), the way hdlc_body.hpp serves k_hdlc_* and k_rx_*.  Tiles are taken from
// blockIdx.x in steps of gridDim.x, so a workgroup whose tiles lie beyond the stream's own count does nothing.
// the one-samples of every audio tile
__device__ __forceinline__ void fsk_count_body(const FskTxArgs& a) {
    __shared__ unsigned s_w[FSK_B / 64];
    const long ntiles = (a.na + FSK_T - 1) / FSK_T;
    for (long tile = blockIdx.x; tile < ntiles; tile += (long)gridDim.x) {
        const long m0 = tile * FSK_T + (long)threadIdx.x * FSK_PER;
        const long left = a.na - m0;
        const unsigned mask = fsk_ones8(a, m0, (int)(left < FSK_PER ? left : FSK_PER));
        unsigned total;
        (void)fsk_block_scan<FSK_B / 64>((unsigned)__popc(mask), s_w, total);
        if (threadIdx.x == 0) a.tilecnt[tile] = total;
    }
}
__global__ __launch_bounds__(FSK_B) void k_fsk_count(FskTxArgs a) { fsk_count_body(a); }

// tilecnt[i] <- tilecnt[0] + ... + tilecnt[i - 1] (at most 2^30: the audio samples of a push).  One workgroup, chunks of
// VCO_SCHUNK tiles, as k_vco_scan.
__device__ __forceinline__ void fsk_scan1_body(unsigned* __restrict__ tilecnt, long ntiles) {
    __shared__ unsigned s_w[VCO_SB / 64];
    unsigned base = 0;
    for (long c0 = 0; c0 < ntiles; c0 += VCO_SCHUNK) {
        const long j0 = c0 + (long)threadIdx.x * VCO_SPER;
        unsigned v[VCO_SPER], run = 0;
#pragma unroll
        for (int i = 0; i < VCO_SPER; ++i) { v[i] = j0 + i < ntiles ? tilecnt[j0 + i] : 0u; run += v[i]; }
        unsigned total;
        unsigned p = base + fsk_block_scan<VCO_SB / 64>(run, s_w, total);
#pragma unroll
        for (int i = 0; i < VCO_SPER; ++i) {
            if (j0 + i < ntiles) tilecnt[j0 + i] = p;
            p += v[i];
        }
        base += total;
    }
}
__global__ __launch_bounds__(VCO_SB) void k_fsk_scan1(unsigned* __restrict__ tilecnt, long ntiles) { fsk_scan1_body(tilecnt, ntiles); }

// Stage 1, and in AFSK mode the audio-rate half of stage 2.  Per audio sample m of the push: its phase from the count of
// one-samples up to it (fsk_phase1), then
//   DIRECT  val[m] = gain * (sin, cos), what the map kernel copies to the sample's outputs
//   AFSK    audio[m] = fl32(fl32(sin) * gain); pre2[m] = the wrapped sum of rep2(m') * (k2 * audio[m']) over the tile's m' < m
//           (SINGLE: on top of the carried phase 2), and the tile's sum to tiles2[tile] (SINGLE: phase 2 carried out)
// The thread that owns the push's last sample writes phase 1 carried out.
template <bool AFSK, bool SINGLE>
__device__ __forceinline__ void fsk_audio_body(const FskTxArgs& a) {
    __shared__ unsigned s_c[FSK_B / 64];
    __shared__ double s_w[FSK_B / 64];
    const long ntiles = (a.na + FSK_T - 1) / FSK_T;
    const double carried1 = a.carry_in[0];
    for (long tile = blockIdx.x; tile < ntiles; tile += (long)gridDim.x) {
        const long m0 = tile * FSK_T + (long)threadIdx.x * FSK_PER;
        const long left = a.na - m0;
        const int cnt = (int)(left < 0 ? 0 : left < FSK_PER ? left : FSK_PER);
        const unsigned mask = fsk_ones8(a, m0, cnt);
        unsigned total1;
        long c1 = (long)fsk_block_scan<FSK_B / 64>((unsigned)__popc(mask), s_c, total1);
        if (!SINGLE) c1 += (long)a.tilecnt[tile];
        FskWalk f2{};
        if (AFSK && cnt > 0) f2 = fsk_walk_first(a.r2, a.e2, m0);
        double e[FSK_PER], run = 0.0;
#pragma unroll
        for (int i = 0; i < FSK_PER; ++i) {
            e[i] = run;
            if (i < cnt) {
                const long m = m0 + i;
                c1 += (mask >> i) & 1u;
                const double ph = fsk_phase1(carried1, c1, m + 1 - c1, a.dhi, a.dlo);
                double sn, cs;
                vco_sincos(ph, &sn, &cs);
                if (m == a.na - 1) a.carry_out[0] = ph;
                if (AFSK) {
                    const float au = (float)sn * a.gain;
                    a.audio[m] = au;
                    const long o0 = f2.q;
                    f2.next();
                    run = vco_wrap(run + fsk_red(f2.q - o0, fsk_step(a.k2, au)));
                } else {
                    a.val[m] = mkcf((float)sn * a.gain, (float)cs * a.gain);
                }
            }
        }
        if (AFSK) {
            double total2;
            double p0 = vco_block_scan<FSK_B / 64>(run, s_w, total2);
            if (SINGLE) p0 = vco_wrap(a.carry_in[1] + p0);
#pragma unroll
            for (int i = 0; i < FSK_PER; ++i)
                if (i < cnt) a.pre2[m0 + i] = vco_wrap(p0 + e[i]);
            if (threadIdx.x == 0) {
                if (SINGLE) a.carry_out[1] = vco_wrap(a.carry_in[1] + total2);
                else a.tiles2[tile] = total2;
            }
        }
    }
}
template <bool AFSK, bool SINGLE>
__global__ __launch_bounds__(FSK_B) void k_fsk_audio(FskTxArgs a) { fsk_audio_body<AFSK, SINGLE>(a); }

// The output-rate kernel: a map.  Output o of the push belongs to audio sample m = src2(o) and is the j-th of its run, j - 1 =
// floor(rem / D2) with rem what the division left; thread t takes o = tile * FSK_OT + t + 256 i, so a wave's stores are one run
// of 512 bytes and m moves by a fixed step: one 64-bit division per thread and tile.
//   DIRECT  out[o] = val[m]
//   AFSK    out[o] = (sin, cos)(base + pre2[m] + j * (k2 * audio[m])), base = tiles2[m's tile] (SINGLE: pre2 holds it already)
template <bool AFSK, bool SINGLE>
__device__ __forceinline__ void fsk_map_body(const FskTxArgs& a) {
    const long ntiles = (a.no + FSK_OT - 1) / FSK_OT;
    for (long tile = blockIdx.x; tile < ntiles; tile += (long)gridDim.x) {
        const long o0 = tile * FSK_OT + threadIdx.x;
        if (o0 >= a.no) continue;             // (no barrier in this kernel)
        FskWalk w = fsk_walk(a.e2 + o0 * a.r2.D, a.map_dq, a.map_dr, a.r2.I);
#pragma unroll
        for (int i = 0; i < FSK_PER; ++i) {
            const long o = o0 + (long)i * FSK_B;
            if (o < a.no) {
                const long m = w.q;
                if (AFSK) {
                    const long j = (long)((unsigned)w.r / (unsigned)a.r2.D) + 1;      // both below 2^32: I2, D2 <= 2^31
                    double p = a.pre2[m];
                    if (!SINGLE) p = vco_wrap(a.tiles2[m / FSK_T] + p);
                    p = vco_wrap(p + fsk_red(j, fsk_step(a.k2, a.audio[m])));
                    double sn, cs;
                    vco_sincos(p, &sn, &cs);
                    a.out[o] = mkcf((float)sn, (float)cs);
                } else {
                    a.out[o] = a.val[m];
                }
                w.next();
            }
        }
    }
}
template <bool AFSK, bool SINGLE>
__global__ __launch_bounds__(FSK_B) void k_fsk_map(FskTxArgs a) { fsk_map_body<AFSK, SINGLE>(a); }

template <bool AFSK> static void fsk_launch(const FskTxArgs& a, hipStream_t s) {
    const long ntiles = (a.na + FSK_T - 1) / FSK_T;
    const unsigned go = tiles_grid((a.no + FSK_OT - 1) / FSK_OT);
    if (ntiles == 1) {
        hipLaunchKernelGGL((k_fsk_audio<AFSK, true>), dim3(1), dim3(FSK_B), 0, s, a);
        if (a.no > 0) hipLaunchKernelGGL((k_fsk_map<AFSK, true>), dim3(go), dim3(FSK_B), 0, s, a);
        RR_HIP(hipGetLastError());
        return;
    }
    const unsigned g = tiles_grid(ntiles);
    hipLaunchKernelGGL(k_fsk_count, dim3(g), dim3(FSK_B), 0, s, a);
    hipLaunchKernelGGL(k_fsk_scan1, dim3(1), dim3(VCO_SB), 0, s, a.tilecnt, ntiles);
    hipLaunchKernelGGL((k_fsk_audio<AFSK, false>), dim3(g), dim3(FSK_B), 0, s, a);
    if (AFSK) hipLaunchKernelGGL(k_vco_scan, dim3(1), dim3(VCO_SB), 0, s, a.tiles2, ntiles, a.carry_in + 1, a.carry_out + 1);
    if (a.no > 0) hipLaunchKernelGGL((k_fsk_map<AFSK, false>), dim3(go), dim3(FSK_B), 0, s, a);
    RR_HIP(hipGetLastError());
}
void launch_fsk_tx(const FskTxArgs& a, bool afsk, hipStream_t s) {
    if (a.na <= 0) return;
    if (afsk) fsk_launch<true>(a, s);
    else fsk_launch<false>(a, s);
}

// ---- rr_fsk_tx_multi: the general path above for nstreams streams, the stream from blockIdx.y -------------------
// One thread per stream plans its push from the FskPos it carries and its clamped count, and writes what no later kernel of the
// push writes: the plan, the next FskPos, the public counts and the phases that stay as they are (both where the push makes no
// audio sample; phase 2 always in DIRECT mode).  Phase 1 of a stream with audio is k_fskm_audio's, its phase 2 k_fskm_scan2's.
__global__ __launch_bounds__(FSK_B) void k_fskm_plan(FskTxMultiArgs m, int afsk) {
    const long c = (long)blockIdx.x * FSK_B + threadIdx.x;
    if (c >= m.nstreams) return;
    unsigned long long k = m.counts ? m.counts[c] : (unsigned long long)m.n_cap;
    if (k > (unsigned long long)m.n_cap) k = (unsigned long long)m.n_cap;
    const FskStream st = m.st_in[c];
    FskPush u = fsk_plan(st.pos, m.r1, m.r2, (long)k);
    // (residues in [0, D) keep a push inside the bound; a state that is not such a one takes nothing rather than write beyond it)
    if (u.no < 0 || u.na > m.audio_cap || u.no > m.out_cap) u = fsk_plan(st.pos, m.r1, m.r2, 0);
    m.plan[c] = u;
    m.st_out[c].pos = u.next;
    if (u.na == 0) m.st_out[c].ph[0] = st.ph[0];
    if (u.na == 0 || !afsk) m.st_out[c].ph[1] = st.ph[1];
    m.made[c] = (unsigned long long)u.na;
    m.made[m.nstreams + c] = (unsigned long long)u.no;
}
// stream c of the push as rr_fsk_tx's kernels see one push: indices relative to the stream's own push start, so nothing below
// depends on n_cap, the strides, nstreams or another stream
__device__ __forceinline__ FskTxArgs fskm_view(const FskTxMultiArgs& m, long c) {
    const FskPush* u = m.plan + c;
    FskTxArgs a;
    a.bits = m.bits + c * m.bits_stride;
    a.n = u->n; a.na = u->na; a.no = u->no;
    a.r1 = m.r1; a.r2 = m.r2;
    a.e1 = u->e1; a.e2 = u->e2;
    a.map_dq = m.map_dq; a.map_dr = m.map_dr;
    a.dhi = m.dhi; a.dlo = m.dlo; a.k2 = m.k2;
    a.gain = m.gain;
    a.carry_in = m.st_in[c].ph;
    a.carry_out = m.st_out[c].ph;
    a.tilecnt = m.tilecnt + c * m.tpitch;
    a.tiles2 = m.tiles2 + c * m.tpitch;
    a.audio = m.audio + c * m.audio_stride;
    a.pre2 = m.pre2 + c * m.audio_cap;
    a.val = m.val + c * m.audio_cap;
    a.out = m.out + c * m.out_stride;
    return a;
}
__global__ __launch_bounds__(FSK_B) void k_fskm_count(FskTxMultiArgs m) { fsk_count_body(fskm_view(m, blockIdx.y)); }
__global__ __launch_bounds__(VCO_SB) void k_fskm_scan1(FskTxMultiArgs m) {
    const FskTxArgs a = fskm_view(m, blockIdx.y);
    fsk_scan1_body(a.tilecnt, (a.na + FSK_T - 1) / FSK_T);
}
template <bool AFSK> __global__ __launch_bounds__(FSK_B) void k_fskm_audio(FskTxMultiArgs m) {
    fsk_audio_body<AFSK, false>(fskm_view(m, blockIdx.y));
}
__global__ __launch_bounds__(VCO_SB) void k_fskm_scan2(FskTxMultiArgs m) {
    const FskTxArgs a = fskm_view(m, blockIdx.y);
    if (a.na <= 0) return;                    // (the plan kernel carried this stream's phase 2 over)
    vco_scan_body(a.tiles2, (a.na + FSK_T - 1) / FSK_T, a.carry_in + 1, a.carry_out + 1);
}
template <bool AFSK> __global__ __launch_bounds__(FSK_B) void k_fskm_map(FskTxMultiArgs m) {
    fsk_map_body<AFSK, false>(fskm_view(m, blockIdx.y));
}

template <bool AFSK> static void fskm_launch(const FskTxMultiArgs& m, hipStream_t s) {
    const unsigned ns = (unsigned)m.nstreams;
    const dim3 ga(tiles_grid(m.tpitch), ns), go(tiles_grid((m.out_cap + FSK_OT - 1) / FSK_OT), ns), one(1, ns);
    hipLaunchKernelGGL(k_fskm_plan, dim3((ns + FSK_B - 1) / FSK_B), dim3(FSK_B), 0, s, m, AFSK ? 1 : 0);
    hipLaunchKernelGGL(k_fskm_count, ga, dim3(FSK_B), 0, s, m);
    hipLaunchKernelGGL(k_fskm_scan1, one, dim3(VCO_SB), 0, s, m);
    hipLaunchKernelGGL((k_fskm_audio<AFSK>), ga, dim3(FSK_B), 0, s, m);
    if (AFSK) hipLaunchKernelGGL(k_fskm_scan2, one, dim3(VCO_SB), 0, s, m);
    hipLaunchKernelGGL((k_fskm_map<AFSK>), go, dim3(FSK_B), 0, s, m);
    RR_HIP(hipGetLastError());
}
void launch_fsk_tx_multi(const FskTxMultiArgs& m, bool afsk, hipStream_t s) {
    if (m.n_cap <= 0 || m.nstreams <= 0) return;
    if (afsk) fskm_launch<true>(m, s);
    else fskm_launch<false>(m, s);
}

}  // namespace rr
