// kernels_wpcr.hip — Wpcr (src/wpcr.rs:105-239), whole-packet clock recovery, over a batch of disjoint bursts inside one f32
// sample buffer.  Per burst x[0 .. n), N = n - 1 (Wpcr::process_one, :130-197, and find_best_bin, :217-239):
//   d[j] = (s[j] - s[j+1])^2, s[j] = x[j] > mid          the zero crossings as a 0/1 pulse train (:141-149)
//   X = DFT_N(d), bins k < N / 2, mag = |X| in f32        (:153-156, :222)
//   bin = the first k >= 2 with mag[k] > 0.8f max(mag[2 ..)) and mag[k] > mag[k + 1]            (:225-238)
//   f = bin / n, p0 = 0.5f + arg X[bin] / 2 pi, + 1 unless > 0.5                               (:165-169)
//   symbols = the samples at which the clock p0 + i f passes an integer                         (:180-186)
// Four launches ordered by the stream alone, the shape of kernels_burst.hip / kernels_bits.hip:
//   k_wpcr_cross    per tile of WPCR_T samples the positions j with d[j] = 1, ascending, into slots the BURST owns (its own
//                   range of a list as long as the sample buffer: tile t's at list[start + t WPCR_T ..)) and their number
//   k_wpcr_dft      d is sparse and 0/1, so X[k] = sum_j e^(-2 pi i (j k mod N) / N) over the crossings.  j k mod N is reduced
//                   EXACTLY in integers before any rounding (j k0 mod N for a tile's first bin once per crossing, f64 holding the
//                   product; from there r0 + j tid < 2^28 in 32 bits, the quotient off by one at most and fixed up), so the
//                   accuracy does not depend on N and every length works without a plan or a table.  A thread owns four bins
//                   256 apart: one sincospif per crossing for the first, and the other three by a complex multiply with
//                   W^(256 m j), which the threads that stage a chunk of crossings in LDS compute once per crossing.  f32 sums
//                   of 16 terms at most, f64 sums of those.
//   k_wpcr_decide   ONE workgroup per burst: max over [2, N / 2), then the LOWEST qualifying bin, then f, p0, nsyms and the end
//                   phase into the burst's result record
//   k_wpcr_gather   per sample: taken iff floor(P(i)) > floor(P(i - 1)), P(i) = p0 + i f evaluated EXACTLY in 64-bit integers
//                   (below); sample i becomes symbol floor(P(i)) - 1 of the burst, written to syms[start + that]
// The grids run over (burst, tile) pairs through tile -> burst maps made on the host, so bursts of very different lengths
// share one launch.  No workgroup waits on another one, no counter is shared between workgroups.
//
// NOT bit-equal to the reference's symbol picks: it accumulates the phase in f32 (phase += f per sample, :185) and drifts off
// p0 + i f by up to i 2^-24; this block evaluates the clock without that drift.  The picks differ only where P(i) or P(i - 1)
// lies within (i + 1) 2^-24 of an integer; there the reference takes the neighbouring sample.
//
// Accuracy of X (the bound of include/rustradio_amd.h): a phase is 2 pi fl32(2 r / N) / 2 with r exact, so a phasor out of
// sincospif is off by pi 2^-23 from that one rounding plus sincospif's own error; a product of two has twice that and its own
// 3 2^-24.  A group of 16 terms adds 15 roundings, the f64 sums add less than 2^-34 C, and they are cast to f32 once.
#include "kernels.hpp"

namespace rr {

constexpr int WPCR_B = 256;                    // threads of every workgroup here
constexpr int WPCR_PER = WPCR_T / WPCR_B;      // consecutive samples of one thread of k_wpcr_cross
constexpr int WPCR_BPT = WPCR_BT / WPCR_B;     // bins of one thread of k_wpcr_dft, WPCR_B apart
constexpr int WPCR_FL = 16;                    // f32 additions between two flushes into the f64 sums
static_assert(WPCR_PER == 8 && WPCR_BPT == 4, "8 samples per thread; 4 bins per thread");

__global__ __launch_bounds__(WPCR_B) void k_wpcr_cross(const float* __restrict__ x, const WpcrBurst* __restrict__ bursts,
                                                       const int* __restrict__ smap, unsigned* __restrict__ list,
                                                       unsigned* __restrict__ tilecnt) {
    __shared__ float s_x[WPCR_T + 1];
    __shared__ int s_w[WPCR_B / 64];
    const WpcrBurst B = bursts[smap[blockIdx.x]];
    const int t = (int)blockIdx.x - B.stile0, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int N = B.n - 1, j0 = t * WPCR_T;
    const int cnt = min(WPCR_T, N - j0);       // pulses of this tile: j0 .. j0 + cnt (<= 0: the burst's last sample alone)
    const float* xb = x + B.start;
    for (int j = threadIdx.x; j <= WPCR_T; j += WPCR_B) s_x[j] = j <= cnt ? xb[j0 + j] : 0.0f;   // one sample of look-ahead
    __syncthreads();
    const int i0 = threadIdx.x * WPCR_PER;
    unsigned m = 0;
    bool prev = s_x[i0] > B.mid;               // NaN: false on either side
#pragma unroll
    for (int i = 0; i < WPCR_PER; ++i) {
        const bool cur = s_x[i0 + i + 1] > B.mid;
        if (i0 + i < cnt && cur != prev) m |= 1u << i;
        prev = cur;
    }
    // exclusive scan of the threads' counts: lanes, then the wave totals
    const int c = __popc(m);
    int inc = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < WPCR_B / 64; ++k) { if (k < w) base += s_w[k]; total += s_w[k]; }
    unsigned* dst = list + B.start + j0 + base + (inc - c);       // (slots < start + j0 + cnt: as many as pulses at most)
    for (int i = 0; i < WPCR_PER; ++i)
        if (m >> i & 1) *dst++ = (unsigned)(j0 + i0 + i);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = (unsigned)total;
}

// j k mod N for j, k < 2^19: p < 2^38 is exact in f64, q is floor(p / N) or one off it, and p - q N is an integer below 2 N in
// magnitude, so the fma is exact and one correction either way finishes it
__device__ __forceinline__ double wpcr_mulmod(double j, double k, double Nd, double invN) {
    const double p = j * k;
    const double q = floor(p * invN);
    double r = fma(-q, Nd, p);
    r += r < 0.0 ? Nd : 0.0;
    r -= r >= Nd ? Nd : 0.0;
    return r;
}

// One crossing as the transform's threads read it (a broadcast of 32 B): j, r0 = j k0 mod N for the tile's first bin k0, and
// W^(256 m j) = (wc[m-1], -ws[m-1]), m = 1 .. 3, the steps from a thread's first bin to its other three
struct alignas(16) WpcrCross {
    unsigned j, r0;
    float wc[WPCR_BPT - 1], ws[WPCR_BPT - 1];
};
static_assert(sizeof(WpcrCross) == 32, "two 16-byte LDS reads");

__global__ __launch_bounds__(WPCR_B) void k_wpcr_dft(const WpcrBurst* __restrict__ bursts, const int* __restrict__ bmap,
                                                     const unsigned* __restrict__ list, const unsigned* __restrict__ tilecnt,
                                                     float* __restrict__ mag, float* __restrict__ reim) {
    __shared__ WpcrCross s_c[WPCR_CH];
    const WpcrBurst B = bursts[bmap[blockIdx.x]];
    const int N = B.n - 1, nb2 = N / 2;
    const int k0 = ((int)blockIdx.x - B.btile0) * WPCR_BT;     // this thread's bins: k0 + tid + WPCR_B m, m < WPCR_BPT
    const int nst = (B.n + WPCR_T - 1) / WPCR_T;
    const double Nd = (double)N, invN = 1.0 / Nd, two_over_N = 2.0 / Nd;
    const float invNf = 1.0f / (float)N;
    double re[WPCR_BPT], im[WPCR_BPT];
#pragma unroll
    for (int m = 0; m < WPCR_BPT; ++m) re[m] = im[m] = 0.0;
    for (int t = 0; t < nst; ++t) {
        const int ct = (int)tilecnt[B.stile0 + t];
        const unsigned* src = list + B.start + (long)t * WPCR_T;
        for (int cb = 0; cb < ct; cb += WPCR_CH) {             // a tile's crossings in chunks of WPCR_CH
            const int c = min(WPCR_CH, ct - cb);
            for (int i = threadIdx.x; i < c; i += WPCR_B) {
                WpcrCross X;
                X.j = src[cb + i];
                X.r0 = (unsigned)wpcr_mulmod((double)X.j, (double)k0, Nd, invN);
                const double rs = wpcr_mulmod((double)X.j, (double)WPCR_B, Nd, invN);
                double rm = 0.0;
#pragma unroll
                for (int m = 0; m < WPCR_BPT - 1; ++m) {
                    rm += rs;                                  // (m + 1) rs mod N: both below N
                    rm -= rm >= Nd ? Nd : 0.0;
                    sincospif((float)(rm * two_over_N), &X.ws[m], &X.wc[m]);
                }
                s_c[i] = X;
            }
            __syncthreads();
            for (int i0 = 0; i0 < c; i0 += WPCR_FL) {          // f32 sums of WPCR_FL terms at most, then into the f64 sums
                float ar[WPCR_BPT], ai[WPCR_BPT];
#pragma unroll
                for (int m = 0; m < WPCR_BPT; ++m) ar[m] = ai[m] = 0.0f;
                const int i1 = min(i0 + WPCR_FL, c);
                for (int i = i0; i < i1; ++i) {
                    // r = j k mod N = (r0 + j tid) mod N in 32-bit integers: v < N + 255 N < 2^28 and v / N < 256, so the f32
                    // quotient is off the true one by less than 256 * 3 * 2^-24 and its integer part by one at most either way.
                    // (j, N < 2^19 and tid, q < 2^9: 24-bit multiplies, which run at the full rate)
                    const WpcrCross X = s_c[i];
                    const unsigned v = X.r0 + __umul24(X.j, threadIdx.x);
                    const unsigned q = (unsigned)((float)v * invNf);
                    int r = (int)v - (int)__umul24(q, (unsigned)N);
                    r += r < 0 ? N : 0;
                    r -= r >= N ? N : 0;
                    float s0, c0;
                    sincospif((float)((double)r * two_over_N), &s0, &c0);     // the ONE rounding of a phase: fl32(2 r / N) in [0, 2)
                    ar[0] += c0;
                    ai[0] -= s0;
#pragma unroll
                    for (int m = 1; m < WPCR_BPT; ++m) {       // e^(-i a) e^(-i b) = (ca cb - sa sb) - i (sa cb + ca sb)
                        ar[m] += fmaf(c0, X.wc[m - 1], -(s0 * X.ws[m - 1]));
                        ai[m] -= fmaf(s0, X.wc[m - 1], c0 * X.ws[m - 1]);
                    }
                }
#pragma unroll
                for (int m = 0; m < WPCR_BPT; ++m) { re[m] += (double)ar[m]; im[m] += (double)ai[m]; }
            }
            __syncthreads();                   // the next chunk overwrites s_c
        }
    }
#pragma unroll
    for (int m = 0; m < WPCR_BPT; ++m) {
        const int k = k0 + (int)threadIdx.x + WPCR_B * m;
        if (k < nb2) {
            const float fr = (float)re[m], fi = (float)im[m];
            mag[B.start + k] = sqrtf(add_rn(mul_rn(fr, fr), mul_rn(fi, fi)));      // norm_sqr().sqrt() (:222), no FMA
            reim[B.start + k] = fr;
            reim[B.start + nb2 + k] = fi;      // (2 nb2 <= N < n: inside the burst's own range)
        }
    }
}

// The clock p0 + i f in exact integers.  f = Mf 2^-S with Mf < 2^24 and S = 150 - (biased exponent of f) in [25, 46] for
// 2^-23 <= f < 0.5; p0 in (0.5, 1.5] is a multiple of 2^-24 = 2^-S 2^(S - 24).  P(i) 2^S = P0 + i Mf < 2^47 + 2^48 for every
// i <= 2^24.
struct WpcrClock {
    unsigned long long P0, Mf;
    int S;
    __device__ __forceinline__ WpcrClock(float p0, float f) {
        const unsigned fb = __float_as_uint(f), pb = __float_as_uint(p0);
        const int Ef = (int)(fb >> 23), Ep = (int)(pb >> 23);     // (both positive and normal)
        Mf = (fb & 0x7fffffu) | 0x800000u;
        S = 150 - Ef;
        P0 = (unsigned long long)((pb & 0x7fffffu) | 0x800000u) << (Ep - Ef);
    }
    // floor(P(i)), i >= 0
    __device__ __forceinline__ unsigned long long fl(long i) const { return (P0 + (unsigned long long)i * Mf) >> S; }
};

__global__ __launch_bounds__(WPCR_B) void k_wpcr_decide(const WpcrBurst* __restrict__ bursts, const float* __restrict__ mag,
                                                        const float* __restrict__ reim, float samp_rate,
                                                        WpcrResult* __restrict__ res) {
    __shared__ float s_max[WPCR_B / 64];
    __shared__ int s_first;
    const WpcrBurst B = bursts[blockIdx.x];
    const int n = B.n, N = n - 1, nb2 = N / 2, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* mg = mag + B.start;
    WpcrResult r;
    r.ok = 0; r.bin = 0; r.sps = 0.0f; r.phase0 = 0.0f; r.phase = 0.0f; r.frequency = 0.0f; r.nsyms = 0;
    if (n < 4 || nb2 < 4) {                    // :131-133, and no k >= 2 with k + 1 < N / 2
        if (threadIdx.x == 0) res[blockIdx.x] = r;
        return;
    }
    float mx = 0.0f;                           // (magnitudes are finite and >= 0)
    for (int k = 2 + threadIdx.x; k < nb2; k += WPCR_B) mx = fmaxf(mx, mg[k]);
#pragma unroll
    for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) s_max[w] = mx;
    if (threadIdx.x == 0) s_first = 0x7fffffff;
    __syncthreads();
    mx = s_max[0];
#pragma unroll
    for (int k = 1; k < WPCR_B / 64; ++k) mx = fmaxf(mx, s_max[k]);
    const float thresh = mul_rn(mx, 0.8f);     // :225-230
    // the LOWEST k: chunks in ascending order, the minimum inside the first chunk that has one
    for (int k0 = 2; k0 < nb2 - 1; k0 += WPCR_B) {
        const int k = k0 + threadIdx.x;
        if (k < nb2 - 1) {
            const float v = mg[k];
            if (v > thresh && v > mg[k + 1]) atomicMin(&s_first, k);
        }
        __syncthreads();
        if (s_first != 0x7fffffff) break;      // (uniform: read after the barrier, written before it)
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int bin = s_first;
    if (bin != 0x7fffffff) {
        const int nb = nb2;
        const float fr = reim[B.start + bin], fi = reim[B.start + nb + bin];
        // bin / n: two integers below 2^24, so the f64 quotient rounds to the correctly rounded f32 one
        const float f = (float)((double)bin / (double)n);
        const float t = add_rn(0.5f, __fdiv_rn(atan2f(fi, fr), 6.2831855f));      // :167
        const float p0 = t > 0.5f ? t : add_rn(t, 1.0f);                           // :168
        const WpcrClock ck(p0, f);
        const unsigned long long ns = ck.fl(n - 1);
        // P(n) - nsyms < 1.5, below 2^(S + 1) in units of 2^-S: one rounding to f32, then an exact scaling
        const unsigned long long D = ck.P0 + (unsigned long long)n * ck.Mf - (ns << ck.S);
        r.ok = 1; r.bin = (unsigned)bin; r.sps = f; r.phase0 = p0;
        r.phase = ldexpf((float)D, -ck.S);
        r.frequency = mul_rn(f, samp_rate);    // :172 (NaN without a sample rate)
        r.nsyms = ns;
    }
    res[blockIdx.x] = r;
}

template <bool MID>
__global__ __launch_bounds__(WPCR_B) void k_wpcr_gather(const float* __restrict__ x, const WpcrBurst* __restrict__ bursts,
                                                        const int* __restrict__ smap, const WpcrResult* __restrict__ res,
                                                        float* __restrict__ syms) {
    const int b = smap[blockIdx.x];
    const WpcrResult r = res[b];
    if (!r.ok) return;
    const WpcrBurst B = bursts[b];
    const WpcrClock ck(r.phase0, r.sps);
    const int i0 = ((int)blockIdx.x - B.stile0) * WPCR_T;
#pragma unroll
    for (int u = 0; u < WPCR_PER; ++u) {
        const int i = i0 + u * WPCR_B + threadIdx.x;
        if (i >= B.n) break;
        const unsigned long long cur = ck.fl(i), prev = i ? ck.fl(i - 1) : 0ull;
        if (cur > prev) {                      // (f < 0.5: by one at most)
            const float v = x[B.start + i];
            syms[B.start + (long)cur - 1] = MID ? sub_rn(v, B.mid) : v;            // cur - 1 < nsyms <= n / 2 + 1 < n
        }
    }
}

void launch_wpcr(const float* x, const WpcrBurst* bursts, long nbursts, const int* smap, long nstiles, const int* bmap, long nbtiles,
                 bool has_mid, float samp_rate, unsigned* list, unsigned* tilecnt, float* mag, float* reim, WpcrResult* res,
                 float* syms, hipStream_t s) {
    if (nbursts <= 0) return;
    if (nstiles) hipLaunchKernelGGL(k_wpcr_cross, dim3((unsigned)nstiles), dim3(WPCR_B), 0, s, x, bursts, smap, list, tilecnt);
    if (nbtiles) hipLaunchKernelGGL(k_wpcr_dft, dim3((unsigned)nbtiles), dim3(WPCR_B), 0, s, bursts, bmap, (const unsigned*)list,
                                    (const unsigned*)tilecnt, mag, reim);
    hipLaunchKernelGGL(k_wpcr_decide, dim3((unsigned)nbursts), dim3(WPCR_B), 0, s, bursts, (const float*)mag, (const float*)reim,
                       samp_rate, res);
    if (nstiles) {
        if (has_mid)
            hipLaunchKernelGGL((k_wpcr_gather<true>), dim3((unsigned)nstiles), dim3(WPCR_B), 0, s, x, bursts, smap,
                               (const WpcrResult*)res, syms);
        else
            hipLaunchKernelGGL((k_wpcr_gather<false>), dim3((unsigned)nstiles), dim3(WPCR_B), 0, s, x, bursts, smap,
                               (const WpcrResult*)res, syms);
    }
    RR_HIP(hipGetLastError());
}

}  // namespace rr
