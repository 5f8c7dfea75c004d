// kernels_burst.hip — ComplexToMag2 (src/complex_to_mag2.rs:8-21), SinglePoleIirFilter (src/single_pole_iir_filter.rs:11-93)
// and the fused burst path of examples/burst_saver.rs:111-123: ComplexToMag2 -> SinglePoleIirFilter -> the comparison of
// BurstTagger (src/burst_tagger.rs:68-85).
//
// The recurrence y[n] = a x[n] + b y[n-1] is a first-order linear scan.  Its element is the affine map y -> b^len y + B of a
// run of `len` samples, B = the run's response to a zero state; two adjacent runs combine as B = B_left b^(len_right) +
// B_right, ONE fma in f64, and because the coefficients are constants the powers of b are tables of the block (made on the
// host in long double).  Three launches ordered by the stream alone, the shape of kernels_tx.hip:
//   k_iir_sums    per full tile of IIR_T samples its zero-state response
//   k_iir_scan    ONE workgroup per row: the tile responses on top of the carried y -> each tile's incoming y, in place
//   k_iir_apply   per tile the scan of its samples from the tile's incoming y, one cast to f32, one store per sample; the
//                 thread that holds the window's last sample writes the y carried out (f64)
// A window of one tile runs k_iir_apply alone.  The burst detector adds the threshold crossings inside every tile to a
// device list in k_iir_apply and the crossings at the tile seams in a fourth, tiny launch (k_iir_seams) that reads the f32
// values the two neighbours actually STORED.
// No workgroup waits on another one: no look-back, no ticket, no spinning on a flag.
//
// All scan arithmetic is f64 fma; a x[n] is exact (24 x 24 bits).  Exclusive prefixes are built from the earlier elements
// only, so a NaN sample reaches its own output and every later one and none before it.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

constexpr int IIR_B = 256;                    // threads of a workgroup
constexpr int IIR_PER = IIR_T / IIR_B;        // consecutive samples of one thread
static_assert(IIR_PER == 8 && IIR_B == 256, "k_iir_apply: 8 samples per thread, 4 waves");
constexpr int IIR_SB = 1024, IIR_SPER = 4, IIR_SCHUNK = IIR_SB * IIR_SPER;   // k_iir_scan: tiles of one chunk
static_assert(IIR_SPER * IIR_T == IIR_SSPAN, "pws is indexed by runs of IIR_SPER tiles");

// The sample behind index i of row `row`.  F32: a strided f32 stream (a Complex stream is two rows one float apart, stride 2).
struct IirSrcF32 {
    const float* p;
    long stride, rs;
    __device__ __forceinline__ float load(int row, long i) const { return p[row * rs + i * stride]; }
};
// MAG2: norm_sqr of a Complex stream with the reference's three f32 roundings (re * re, im * im, their sum; no FMA)
struct IirSrcMag2 {
    const cf* p;
    long rs;
    __device__ __forceinline__ float load(int row, long i) const {
        const cf z = p[row * rs + i];
        return add_rn(mul_rn(z.x, z.x), mul_rn(z.y, z.y));
    }
};

// Exclusive scan over a workgroup of NW waves of one run per thread, every run S samples long: the zero-state response of
// the runs of all EARLIER threads, at this thread's first sample.  pw[k] = b^(S k), k <= 64 NW.  s_w, s_x: NW doubles each.
// Roundings on a path: 6 (lanes) + log2 NW (waves) + 1.
template <int NW> __device__ __forceinline__ double iir_block_scan(double v, const double* __restrict__ pw, double* s_w, double* s_x) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double u = __shfl_up(inc, off, 64);
        if (lane >= off) inc = fma(u, pw[off], inc);          // the run held here is `off` threads long
    }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    if (w == 0) {                                             // the wave totals, scanned the same way by one wave
        double t = lane < NW ? s_w[lane] : 0.0;
#pragma unroll
        for (int off = 1; off < NW; off <<= 1) {
            const double u = __shfl_up(t, off, 64);
            if (lane >= off) t = fma(u, pw[64 * off], t);
        }
        double e = __shfl_up(t, 1, 64);
        if (lane == 0) e = 0.0;
        if (lane < NW) s_x[lane] = e;
    }
    __syncthreads();
    return fma(s_x[w], pw[lane], exc);                        // (wave 0: 0 * pw + exc, exact)
}

template <class SRC>
__global__ __launch_bounds__(IIR_B) void k_iir_sums(SRC src, long n, double a, double b, const double* __restrict__ pw8,
                                                    double* __restrict__ tiles, long tiles_rs) {
    __shared__ double s_w[IIR_B / 64];
    const long nfull = (n + IIR_T - 1) / IIR_T - 1;           // every tile but the last is full; the last one's response is never used
    const int row = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long tile = blockIdx.x; tile < nfull; tile += gridDim.x) {
        const long i0 = tile * IIR_T + (long)threadIdx.x * IIR_PER;
        double r = 0.0;
#pragma unroll
        for (int i = 0; i < IIR_PER; ++i) r = fma(b, r, a * (double)src.load(row, i0 + i));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {              // B = B_left b^(len_right) + B_right, both partners alike
            const double u = __shfl_xor(r, off, 64);
            r = (lane & off) ? fma(u, pw8[off], r) : fma(r, pw8[off], u);
        }
        if (lane == 0) s_w[w] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = s_w[0];
#pragma unroll
            for (int j = 1; j < IIR_B / 64; ++j) t = fma(t, pw8[64], s_w[j]);
            tiles[row * tiles_rs + tile] = t;
        }
        __syncthreads();                      // s_w is free again
    }
}

// tiles[t] <- y at the sample before tile t: the carried y for t = 0, then tiles[t] = tiles[t - 1] b^IIR_T + response[t - 1].
// One workgroup per row walks the tile responses in chunks of IIR_SCHUNK through LDS (1e8 samples are 12 chunks).
// pws[k] = b^(IIR_SSPAN k), k <= IIR_SB; bT = b^IIR_T.
__global__ __launch_bounds__(IIR_SB) void k_iir_scan(double* __restrict__ tiles, long tiles_rs, long ntiles, const double* __restrict__ pws,
                                                     double bT, const double* __restrict__ y_in) {
    __shared__ double s_t[IIR_SCHUNK];
    __shared__ double s_w[IIR_SB / 64], s_x[IIR_SB / 64];
    __shared__ double s_next;
    double* tl = tiles + blockIdx.x * tiles_rs;
    double base = y_in[blockIdx.x];
    for (long c0 = 0; c0 < ntiles; c0 += IIR_SCHUNK) {
        const int cnt = (int)(ntiles - c0 < IIR_SCHUNK ? ntiles - c0 : IIR_SCHUNK);
        for (int j = threadIdx.x; j < IIR_SCHUNK; j += IIR_SB) s_t[j] = c0 + j < ntiles - 1 ? tl[c0 + j] : 0.0;
        __syncthreads();
        double* mine = s_t + threadIdx.x * IIR_SPER;
        double m[IIR_SPER], run = 0.0;
#pragma unroll
        for (int i = 0; i < IIR_SPER; ++i) { m[i] = mine[i]; run = fma(run, bT, m[i]); }
        const double prefix = iir_block_scan<IIR_SB / 64>(run, pws, s_w, s_x);
        double v = fma(base, pws[threadIdx.x], prefix);
#pragma unroll
        for (int i = 0; i < IIR_SPER; ++i) { mine[i] = v; v = fma(v, bT, m[i]); }   // exclusive: earlier tiles only
        if (threadIdx.x == IIR_SB - 1) s_next = v;            // y after the chunk's last tile
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += IIR_SB) tl[c0 + j] = s_t[j];
        base = s_next;
        __syncthreads();                      // the next chunk overwrites s_t and s_next
    }
}

// The burst detector's part of a call (list == nullptr: none).  An entry is (pos << 1) | cur.
struct IirEdges {
    float thr;
    const int* flag_in;                       // cur(-1): the comparison on the last f32 of the previous call
    int* flag_out;
    unsigned long long* count;                // entries of this call (zero on entry)
    unsigned long long* count_next;           // the counter of the NEXT call: zeroed here, on the call's stream
    unsigned long long* list;                 // one slot per sample of the window
    unsigned long long cap;                   // ... so this many: never reached
};

// SINGLE: the window is one tile — y_in[row] is the tile's incoming y.
template <class SRC, bool SINGLE, bool EDGES>
__global__ __launch_bounds__(IIR_B) void k_iir_apply(SRC src, float* __restrict__ out, long out_stride, long out_rs, long n, double a,
                                                     double b, const double* __restrict__ pw8, const double* __restrict__ base,
                                                     long base_rs, const double* __restrict__ y_in, double* __restrict__ y_out,
                                                     IirEdges ed) {
    // the tile's samples, then its outputs, so that both are coalesced in HBM whatever the window's alignment; one pad per
    // thread (8 elements) keeps the threads' own runs on different LDS banks
    __shared__ float s_buf[IIR_T + IIR_B];
    __shared__ double s_w[IIR_B / 64], s_x[IIR_B / 64];
    const int row = blockIdx.y;
    const long ntiles = (n + IIR_T - 1) / IIR_T;
    if (EDGES && blockIdx.x == 0 && threadIdx.x == 0) ed.count_next[0] = 0;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long o0 = tile * IIR_T;
        const int cnt = (int)(n - o0 < IIR_T ? n - o0 : IIR_T);
        for (int j = threadIdx.x; j < IIR_T; j += IIR_B) s_buf[j + j / IIR_PER] = j < cnt ? src.load(row, o0 + j) : 0.0f;
        __syncthreads();
        const int i0 = threadIdx.x * IIR_PER, l0 = threadIdx.x * (IIR_PER + 1);
        float x[IIR_PER];
        double r = 0.0;
#pragma unroll
        for (int i = 0; i < IIR_PER; ++i) { x[i] = s_buf[l0 + i]; r = fma(b, r, a * (double)x[i]); }   // (past cnt: only later threads see it)
        const double prefix = iir_block_scan<IIR_B / 64>(r, pw8, s_w, s_x);
        double y = fma(SINGLE ? y_in[row] : base[row * base_rs + tile], pw8[threadIdx.x], prefix);
#pragma unroll
        for (int i = 0; i < IIR_PER; ++i) {
            y = fma(b, y, a * (double)x[i]);
            const float f = (float)y;
            s_buf[l0 + i] = f;                                // (a slot only this thread has read)
            if (o0 + i0 + i == n - 1) {                       // the window's last sample: what the next call starts from
                y_out[row] = y;
                if (EDGES) ed.flag_out[0] = f > ed.thr ? 1 : 0;
            }
        }
        __syncthreads();
        for (int j0 = 0; j0 < IIR_T; j0 += IIR_B) {
            const int j = j0 + threadIdx.x;
            const bool in = j < cnt;
            const float v = in ? s_buf[j + j / IIR_PER] : 0.0f;
            if (in) out[row * out_rs + (o0 + j) * out_stride] = v;
            if (EDGES) {
                // cur(i) on the f32 that is stored; sample 0 of a later tile is k_iir_seams' (it needs the neighbour's stored f32)
                bool have = in, prev = false;
                if (j == 0) { if (tile == 0) prev = ed.flag_in[0] != 0; else have = false; }
                else if (in) prev = s_buf[(j - 1) + (j - 1) / IIR_PER] > ed.thr;
                const bool cur = v > ed.thr;
                wave_append(have && cur != prev, ((unsigned long long)(o0 + j) << 1) | (cur ? 1ull : 0ull), ed.count, ed.list, ed.cap);
            }
        }
        __syncthreads();                      // the next tile overwrites s_buf
    }
}

// the crossings between out[t IIR_T - 1] and out[t IIR_T], t = 1 .. ntiles - 1, on the values k_iir_apply stored
__global__ __launch_bounds__(IIR_B) void k_iir_seams(const float* __restrict__ out, long ntiles, IirEdges ed) {
    const long t = (long)blockIdx.x * IIR_B + threadIdx.x + 1;
    bool e = false, cur = false;
    if (t < ntiles) {
        cur = out[t * IIR_T] > ed.thr;
        e = cur != (out[t * IIR_T - 1] > ed.thr);
    }
    wave_append(e, ((unsigned long long)(t * IIR_T) << 1) | (cur ? 1ull : 0ull), ed.count, ed.list, ed.cap);
}

template <class SRC, bool EDGES>
static void iir_launch(SRC src, float* out, long out_stride, long out_rs, int rows, long n, const IirCoef& c, const double* y_in,
                       double* y_out, double* tiles, const IirEdges& ed, hipStream_t s) {
    if (n <= 0) return;
    const long ntiles = (n + IIR_T - 1) / IIR_T;
    if (ntiles == 1) {
        hipLaunchKernelGGL((k_iir_apply<SRC, true, EDGES>), dim3(1, rows), dim3(IIR_B), 0, s, src, out, out_stride, out_rs, n, c.a, c.b,
                           c.pw8, (const double*)nullptr, 0L, y_in, y_out, ed);
        RR_HIP(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL((k_iir_sums<SRC>), dim3(tiles_grid(ntiles - 1), rows), dim3(IIR_B), 0, s, src, n, c.a, c.b, c.pw8, tiles, ntiles);
    hipLaunchKernelGGL(k_iir_scan, dim3(rows), dim3(IIR_SB), 0, s, tiles, ntiles, ntiles, c.pws, c.bT, y_in);
    hipLaunchKernelGGL((k_iir_apply<SRC, false, EDGES>), dim3(tiles_grid(ntiles), rows), dim3(IIR_B), 0, s, src, out, out_stride, out_rs, n,
                       c.a, c.b, c.pw8, (const double*)tiles, ntiles, y_in, y_out, ed);
    if (EDGES)
        hipLaunchKernelGGL(k_iir_seams, dim3((unsigned)((ntiles - 1 + IIR_B - 1) / IIR_B)), dim3(IIR_B), 0, s, (const float*)out, ntiles, ed);
    RR_HIP(hipGetLastError());
}

void launch_iir_f32(const float* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles,
                    hipStream_t s) {
    iir_launch<IirSrcF32, false>(IirSrcF32{in, 1, 0}, out, 1, 0, 1, n, c, y_in, y_out, tiles, IirEdges{}, s);
}
void launch_iir_c32(const cf* in, cf* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles, hipStream_t s) {
    iir_launch<IirSrcF32, false>(IirSrcF32{reinterpret_cast<const float*>(in), 2, 1}, reinterpret_cast<float*>(out), 2, 1, 2, n, c,
                                 y_in, y_out, tiles, IirEdges{}, s);
}
void launch_mag2_iir(const cf* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles,
                     hipStream_t s) {
    iir_launch<IirSrcMag2, false>(IirSrcMag2{in, 0}, out, 1, 0, 1, n, c, y_in, y_out, tiles, IirEdges{}, s);
}
void launch_burst_detector(const cf* in, float* out, long n, const IirCoef& c, const double* y_in, double* y_out, double* tiles,
                           float thr, const int* flag_in, int* flag_out, unsigned long long* count, unsigned long long* count_next,
                           unsigned long long* list, hipStream_t s) {
    iir_launch<IirSrcMag2, true>(IirSrcMag2{in, 0}, out, 1, 0, 1, n, c, y_in, y_out, tiles,
                                 IirEdges{thr, flag_in, flag_out, count, count_next, list, (unsigned long long)n}, s);
}

__global__ __launch_bounds__(256) void k_mag2(const cf* __restrict__ in, float* __restrict__ out, long n) {
    const IirSrcMag2 src{in, 0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = src.load(0, i);
}
void launch_mag2(const cf* in, float* out, long n, hipStream_t s) {
    if (n <= 0) return;
    const long blocks = std::min<long>((n + 255) / 256, (long)device_cu_count() * 16);
    hipLaunchKernelGGL(k_mag2, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
