// am_core.hpp — the arithmetic and the indexing k_am of kernels_am.hip shares with the host: plain functions, no HIP types, so
// tests/cpp/emu_am.cpp compiles them with g++ and takes them tile by tile and thread by thread.  The audio path
// of examples/airspy_am_decode.rs:
//   Map(|v| v.norm()) -> FftFilterFloat as its definition (src/fft_filter.rs:365-491) -> RationalResampler(I : D)
//   (src/rational_resampler.rs:183-198) -> MultiplyConst(scale) (src/multiply_const.rs:20-22)
// per stream, x = every Complex sample so far, L taps, I : D reduced:
//   m[k]   = fl32(sqrt(f64(x[k].re)^2 + f64(x[k].im)^2))             the squares are exact in f64: one add, one sqrt, one narrowing
//   y[p]   = sum_j taps[j] m[p - j]                                   m[< 0] = 0
//   out[o] = scale * y[floor(o D / I)]
// ONE order of operations per output, whatever tile, lane or push it falls into, a function of L alone:
//   s[l]   = the sum over j = l, l + 64, l + 128, .. < L ascending, one fmaf each, from +0          l = 0 .. 63
//   y      = the tree s[l] += s[l ^ 32], then ^ 16, 8, 4, 2, 1 (six levels of f32 adds; each level leaves both partners the
//            same value, so after the last every l holds y)
//   out    = scale * y, one f32 multiply, last
// Only the y the resampler picks are computed: nothing is filtered that is thrown away.
//
// A tile is T = 32 NG outputs of one stream taken by a workgroup of 4 waves; wave w takes the groups 4 g + w (g < NG) of 8
// consecutive outputs, a lane one residue of j.  The taps go by in chunks of KC (a multiple of 64): per chunk the workgroup
// stages the magnitudes the chunk needs in LDS, once, and every lane then adds its terms of the chunk to its 8 NG partial
// sums, which live in registers across the chunks.  Two stagings, chosen at create from (I, D, L):
//   dense    S[q] = m[lo + q], lo = p(first output) - j0 - KC + 1: one run of span + KC magnitudes shared by the whole tile
//            (every magnitude is computed once per tile and chunk, whatever the overlap of the outputs' windows)
//   sparse   S[r KC + q] = m[p(output r) - j0 - KC + 1 + q]: a run of KC per output, for D / I so large that one run over the
//            tile would not fit (the windows of neighbouring outputs are far apart)
// In both, term j of output r reads S[base(r) - (j - j0)]: lanes read descending consecutive floats, no bank is hit twice.
// Positions are relative to the push: output k of the push sits over sample floor((e + k D) / I) of the push, e = O0 D - N0 I in
// [0, D) kept by the host, so no product grows with the stream's age; everything that can pass 2^31 is 64-bit.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define RR_AM_HD __host__ __device__ __forceinline__
#else
#define RR_AM_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define AM_MUL(a, b) ::rr::mul_rn((a), (b))
#define AM_ADD(a, b) ::rr::add_rn((a), (b))
#else
#define AM_MUL(a, b) ((a) * (b))
#define AM_ADD(a, b) ((a) + (b))
#endif
#define AM_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

namespace rr {

constexpr int AM_NT = 256;                    // threads of a workgroup
constexpr int AM_WAVES = 4;
constexpr int AM_G = 8;                       // outputs of a group
constexpr int AM_NG_MAX = 6;                  // groups of a wave: a tile is at most 192 outputs
constexpr int AM_MAX_TAPS = 16384;            // (low_pass(2.5e6, 48000, 500) has 12,045)
constexpr int AM_LDS_FLOATS = 14336;          // S: 56 KiB, two workgroups to a CU
constexpr int AM_KC_DENSE = 4096;             // taps of a chunk at most, dense
constexpr int AM_KC_SPARSE = 448;             // ... sparse: 32 outputs' runs fit S

// What (I, D, L) fix.
struct AmGeom {
    int L;
    int C;                                    // carried magnitudes of a stream: L - 1
    int KC;                                   // taps of a chunk, a multiple of 64
    int NG;                                   // groups of a wave
    int T;                                    // outputs of a tile: 32 NG
    int sparse;
    long I, D;                                // reduced
};
// samples between the first and the last of T consecutive outputs, at most
inline long am_span(long T, long I, long D) { return (long)(((unsigned long long)(T - 1) * (unsigned long long)D + (unsigned long long)(I - 1)) / (unsigned long long)I); }
inline AmGeom am_geom(int L, long I, long D) {
    AmGeom g{};
    g.L = L; g.C = L - 1; g.I = I; g.D = D;
    const int L64 = (L + 63) & ~63;
    g.KC = L64 < AM_KC_DENSE ? L64 : AM_KC_DENSE;
    for (g.NG = AM_NG_MAX; g.NG >= 1; g.NG--)
        if (am_span(32L * g.NG, I, D) + 1 + g.KC <= (long)AM_LDS_FLOATS) break;
    if (g.NG < 1) {
        g.sparse = 1;
        g.KC = L64 < AM_KC_SPARSE ? L64 : AM_KC_SPARSE;
        g.NG = AM_LDS_FLOATS / (32 * g.KC);
        if (g.NG > AM_NG_MAX) g.NG = AM_NG_MAX;
    }
    g.T = 32 * g.NG;
    return g;
}

// One push as the kernel sees it.
struct AmArgs {
    const float* in;                          // stream c: n Complex samples (re, im) at in + 2 c in_stride
    long in_stride, n;
    float* out;                               // stream c: `produced` outputs at out + c out_stride
    long out_stride, produced;
    const float* carry_in;                    // stream c: C magnitudes at carry_in + c C, the stream's latest (zeros before its start)
    float* carry_out;                         // (the other buffer of the pair)
    const float* taps;                        // L
    float scale;
    long e;                                   // output k of the push sits over sample (e + k D) / I of the push
    AmGeom g;
};
// Where a stream that has taken N0 samples stands: e = ceil(N0 I / D) D - N0 I, in [0, D).  A push of n samples behind it:
inline long am_produced(long e, long n, long I, long D) { return n * I > e ? (n * I - e + D - 1) / D : 0; }
inline long am_next_e(long e, long n, long produced, long I, long D) { return e + produced * D - n * I; }
inline long am_tiles(const AmGeom& g, long produced) { return produced > 0 ? (produced + g.T - 1) / g.T : 1; }   // (the carry needs one)

RR_AM_HD float am_mag(float re, float im) {
    const double a = (double)re, b = (double)im;
    return (float)sqrt(a * a + b * b);
}
// m at sample i of the push (i < 0: the carry; before it, and beyond the push, 0)
RR_AM_HD float am_v(const AmArgs& a, long c, long i) {
    if (i >= 0) {
        if (i >= a.n) return 0.0f;
        const float* x = a.in + 2 * (c * a.in_stride + i);
        return am_mag(x[0], x[1]);
    }
    return i >= -(long)a.g.C ? a.carry_in[c * a.g.C + a.g.C + i] : 0.0f;
}
RR_AM_HD long am_pos(const AmArgs& a, long k) { return (long)((unsigned long long)(a.e + k * a.g.D) / (unsigned long long)a.g.I); }
// outputs of tile tx that exist
RR_AM_HD int am_tile_nk(const AmArgs& a, long tx) {
    const long left = a.produced - tx * a.g.T;
    return left <= 0 ? 0 : (left < a.g.T ? (int)left : a.g.T);
}
RR_AM_HD void am_carry(const AmArgs& a, long c, int tid) {
    for (int q = tid; q < a.g.C; q += AM_NT) a.carry_out[c * a.g.C + q] = am_v(a, c, a.n - a.g.C + q);
}
// S for the chunk of taps that starts at j0, thread tid's share
RR_AM_HD void am_stage(const AmArgs& a, long c, long tx, int nk, int j0, int tid, float* S) {
    const long k0 = tx * a.g.T;
    const int KC = a.g.KC;
    if (!a.g.sparse) {
        const long pf = am_pos(a, k0);
        const int len = (int)(am_pos(a, k0 + nk - 1) - pf) + KC;
        const long lo = pf - j0 - (KC - 1);
        for (int q = tid; q < len; q += AM_NT) S[q] = am_v(a, c, lo + q);
    } else {
        for (int r = 0; r < nk; r++) {
            const long lo = am_pos(a, k0 + r) - j0 - (KC - 1);
            for (int q = tid; q < KC; q += AM_NT) S[r * KC + q] = am_v(a, c, lo + q);
        }
    }
}
// S index of term j0 of output r of the tile (r < nk)
RR_AM_HD int am_base(const AmArgs& a, long tx, int r) {
    if (a.g.sparse) return r * a.g.KC + a.g.KC - 1;
    const long k0 = tx * a.g.T;
    return (int)(am_pos(a, k0 + r) - am_pos(a, k0)) + a.g.KC - 1;
}
// One lane's terms of the chunk at j0 for the 8 outputs of one group: acc[u] += taps[j] S[base[u] - (j - j0)], j = j0 + lane + 64 i
RR_AM_HD void am_accum(const AmArgs& a, int j0, int lane, const int base[AM_G], const float* S, float acc[AM_G]) {
    const int L = a.g.L;
    const int jend = j0 + a.g.KC < L ? j0 + a.g.KC : L;                // the chunk's taps: [j0, jend)
    const int nfull = (jend - j0) >> 6;                                // steps every lane takes
    const float* tp = a.taps + j0 + lane;
    int off = lane;
    for (int i = 0; i < nfull; i++, off += 64) {
        const float t = tp[64 * i];
#pragma unroll
        for (int u = 0; u < AM_G; u++) acc[u] = AM_FMA(t, S[base[u] - off], acc[u]);
    }
    if (j0 + off < jend) {                                             // the last, partial step
        const float t = tp[64 * nfull];
#pragma unroll
        for (int u = 0; u < AM_G; u++) acc[u] = AM_FMA(t, S[base[u] - off], acc[u]);
    }
}
// The tree, on the host: v = the 64 lanes' partial sums -> y
inline float am_tree(float v[64]) {
    for (int d = 32; d >= 1; d >>= 1) {
        float w[64];
        for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ d];
        for (int l = 0; l < 64; l++) v[l] = w[l];
    }
    return v[0];
}
RR_AM_HD float am_scale(const AmArgs& a, float y) { return AM_MUL(a.scale, y); }

}  // namespace rr
