// afsk_core.hpp — the arithmetic and the indexing k_afsk of kernels_afsk.hip shares with the host: plain functions, no HIP types,
// so tests/cpp/emu_afsk.cpp compiles them with g++ and takes them thread by thread.  The tone demodulator of the
// 1200-baud receivers (examples/ax25-1200-rx.rs:238-247, il2p-1200-rx.rs:81-89):
//   Hilbert (src/hilbert.rs:38-61,113-116) -> QuadratureDemod (src/quadrature_demod.rs:65-109) -> FftFilterFloat as its
//   definition, y[i] = sum_j taps[j] d[i - j] (src/fft_filter.rs:365-491) -> AddConst (src/add_const.rs:51-68)
// per stream, x = every sample so far, H = hilbert taps, L = low-pass taps, hr[j] = hilbert_taps[H - 1 - j]:
//   xp     = H zeros ++ x
//   a[m]   = (xp[m + H/2], sum_j hr[j] xp[m + j])                  j = 0 .. H-1 ascending, one fmaf each, from +0
//   d[m]   = gain * atan2(Im, Re) of conj(a[m]) a[m+1]             num-complex order, every operation rounded on its own; d[<0] = 0
//   out[i] = (sum_j taps[j] d[i - j]) + offset                     j = 0 .. L-1 ascending, one fmaf each, from +0; one add, last
// ONE order of operations per output, whatever tile, thread or push it falls into: that is the whole of the bit-identity.  All H
// Hilbert taps are used, the zero ones too: 0 * NaN is the reference's NaN, and a NaN sample then reaches exactly the H + L outputs
// whose windows hold it.
//
// A tile is AFSK_TILE outputs of one stream taken by AFSK_NT threads, AFSK_R consecutive outputs each.  The virtual stream V of a
// push is the handle's carry (C = L + H samples, zeros at the start: they are xp's zeros) ++ the push's n samples; output k of the
// push sits at V[s0 + k] and reads V[s0 + k - C + 1 .. s0 + k].  Per tile:
//   afsk_load      X[p] = V[vx0 + p] (zero beyond the push), hr, the front pad of D; the last tile also writes the next carry
//   afsk_demod     groups of 8 consecutive d: 9 Hilbert sums from a sliding register window over X, then the 8 angles into D
//   (the taps then take X's place)
//   afsk_lowpass   each thread's 8 outputs from a sliding register window over D, one LDS read per tap feeding 8 fmaf
// X and D are skewed by one float per 32 (afsk_sk): lanes 8 floats apart then fall on 32 different banks, and an 8-aligned run of 8
// never crosses a skew step, so a chunk's loads are one address plus immediates.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define RR_AFSK_HD __host__ __device__ __forceinline__
#else
#define RR_AFSK_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define AFSK_MUL(a, b) ::rr::mul_rn((a), (b))
#define AFSK_ADD(a, b) ::rr::add_rn((a), (b))
#define AFSK_SUB(a, b) ::rr::sub_rn((a), (b))
#define AFSK_ATAN2(y, x) atan2f((y), (x))
#else
#define AFSK_MUL(a, b) ((a) * (b))
#define AFSK_ADD(a, b) ((a) + (b))
#define AFSK_SUB(a, b) ((a) - (b))
#define AFSK_ATAN2(y, x) std::atan2((y), (x))
#endif
#define AFSK_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

namespace rr {

constexpr int AFSK_TILE = 2048;               // outputs of one tile
constexpr int AFSK_NT = 256;                  // threads of a workgroup
constexpr int AFSK_R = 8;                     // consecutive outputs of one thread (AFSK_TILE = AFSK_NT * AFSK_R)
constexpr int AFSK_MAX_TAPS = 4096;           // low-pass taps of a handle (low_pass(50000, 1100, 100) has 1205)
constexpr int AFSK_MAX_HILBERT = 1023;        // (a deviation: the reference has no cap; the examples use 65)

// What H and L fix: sizes in floats of the tile's LDS regions and where they start.
struct AfskGeom {
    int H, L;
    int C;                                    // carried samples of a stream: L + H
    int NG;                                   // groups of 8 d of a full tile: ceil((AFSK_TILE + L - 1) / 8)
    int padD;                                 // floats in front of d[0] in D: 16 .. 23, (L - 1 + padD) % 8 == 0
    int nx;                                   // entries of X (before the skew)
    int x_floats, d_floats;                   // the regions' sizes; X at 0, D behind it, hr behind D
    int lds_floats;
};
RR_AFSK_HD int afsk_sk(int p) { return p + (p >> 5); }
inline AfskGeom afsk_geom(int H, int L) {
    AfskGeom g{};
    g.H = H; g.L = L;
    g.C = L + H;
    g.NG = (AFSK_TILE + L - 1 + 7) / 8;
    g.padD = 16 + ((8 - (L - 1) % 8) % 8);
    g.nx = 8 * g.NG + (H & ~7) + 16;          // afsk_demod's last chunk loads up to 8 (NG - 1) + (H & ~7) + 15
    g.x_floats = (afsk_sk(g.nx) + 4) & ~3;    // (>= L: the taps take its place)
    g.d_floats = (afsk_sk(8 * g.NG + g.padD) + 4) & ~3;
    g.lds_floats = g.x_floats + g.d_floats + ((H + 3) & ~3);
    return g;
}

// One push as the kernel sees it.
struct AfskArgs {
    const float* in;                          // stream c: n samples at in + c in_stride
    long in_stride, n;
    float* out;                               // stream c: `produced` outputs at out + c out_stride
    long out_stride, produced;
    const float* carry_in;                    // stream c: C samples at carry_in + c C, the stream's latest (zeros before its start)
    float* carry_out;                         // (the other buffer of the pair)
    const float* taps;                        // L
    const float* hr;                          // H, reversed
    float gain, offset;
    long zero_d;                              // d local q of tile k0 is before the stream (d = 0) iff k0 + q < zero_d
    int s0;                                   // output k sits at V[s0 + k]: C for the stream's first push, C - 1 after it
    AfskGeom g;
};
// Geometry of a push of n samples on a stream that has taken `before` so far (the same for every stream of a handle).
inline void afsk_plan(AfskArgs& a, unsigned long long before, long n) {
    a.n = n;
    a.produced = before ? n : (n > 0 ? n - 1 : 0);
    a.s0 = before ? a.g.C - 1 : a.g.C;
    const unsigned long long o0 = before ? before - 1 : 0;            // the stream's index of the push's first output
    a.zero_d = o0 >= (unsigned long long)(a.g.L - 1) ? 0 : (long)(a.g.L - 1) - (long)o0;
}
inline long afsk_tiles(long produced) { return produced > 0 ? (produced + AFSK_TILE - 1) / AFSK_TILE : 1; }   // (the carry needs one)

RR_AFSK_HD float afsk_v(const AfskArgs& a, long c, long v) {
    if (v < a.g.C) return a.carry_in[c * a.g.C + v];
    const long i = v - a.g.C;
    return i < a.n ? a.in[c * a.in_stride + i] : 0.0f;
}
// outputs of tile tx that exist
RR_AFSK_HD int afsk_tile_nk(const AfskArgs& a, long tx) {
    const long left = a.produced - tx * AFSK_TILE;
    return left <= 0 ? 0 : (left < AFSK_TILE ? (int)left : AFSK_TILE);
}
// groups of d those need
RR_AFSK_HD int afsk_tile_groups(const AfskArgs& a, int nk) { return nk ? (nk + a.g.L - 1 + 7) / 8 : 0; }

RR_AFSK_HD void afsk_load(const AfskArgs& a, long c, long tx, bool last, int tid, float* X, float* D, float* HR) {
    if (last)
        for (int j = tid; j < a.g.C; j += AFSK_NT) a.carry_out[c * a.g.C + j] = afsk_v(a, c, a.n + j);
    const int ng = afsk_tile_groups(a, afsk_tile_nk(a, tx));
    if (!ng) return;
    const long vx0 = (long)a.s0 + tx * AFSK_TILE - (a.g.L - 1) - a.g.H;          // >= 0
    const int nx = 8 * ng + (a.g.H & ~7) + 16;
    for (int p = tid; p < nx; p += AFSK_NT) X[afsk_sk(p)] = afsk_v(a, c, vx0 + p);
    for (int j = tid; j < a.g.H; j += AFSK_NT) HR[j] = a.hr[j];
    for (int p = tid; p < a.g.padD; p += AFSK_NT) D[afsk_sk(p)] = 0.0f;
}

// d[8 g .. 8 g + 7] of the tile whose first output is k0
RR_AFSK_HD void afsk_demod(const AfskArgs& a, long k0, int g, const float* X, const float* HR, float* D) {
    const int H = a.g.H, Hc = H & ~7, q0 = 8 * g;
    float e[16], A[9];                        // e[k] = X[q0 + j + k]
    {
        const int b0 = afsk_sk(q0), b1 = afsk_sk(q0 + 8);
#pragma unroll
        for (int k = 0; k < 8; k++) { e[k] = X[b0 + k]; e[8 + k] = X[b1 + k]; }
    }
#pragma unroll
    for (int r = 0; r < 9; r++) A[r] = 0.0f;
    for (int j = 0; j < Hc; j += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const float h = HR[j + u];
#pragma unroll
            for (int r = 0; r < 9; r++) A[r] = AFSK_FMA(h, e[r + u], A[r]);
        }
        const int nb = afsk_sk(q0 + j + 16);
#pragma unroll
        for (int k = 0; k < 8; k++) { e[k] = e[8 + k]; e[8 + k] = X[nb + k]; }
    }
#pragma unroll
    for (int u = 0; u < 7; u++) {
        if (u < H - Hc) {
            const float h = HR[Hc + u];
#pragma unroll
            for (int r = 0; r < 9; r++) A[r] = AFSK_FMA(h, e[r + u], A[r]);
        }
    }
    float re[9];
#pragma unroll
    for (int r = 0; r < 9; r++) re[r] = X[afsk_sk(q0 + r + H / 2)];              // hilbert.rs:115
#pragma unroll
    for (int r = 0; r < 8; r++) {
        // conj(a[m]) * a[m+1] in num-complex order, as k_quaddemod
        const float na = -A[r];
        const float pr = AFSK_SUB(AFSK_MUL(re[r], re[r + 1]), AFSK_MUL(na, A[r + 1]));
        const float pi = AFSK_ADD(AFSK_MUL(re[r], A[r + 1]), AFSK_MUL(na, re[r + 1]));
        float d = AFSK_MUL(a.gain, AFSK_ATAN2(pi, pr));
        if (k0 + q0 + r < a.zero_d) d = 0.0f;
        D[afsk_sk(a.g.padD + q0 + r)] = d;
    }
}

// outputs 8 tid .. 8 tid + 7 of the tile; TP = the taps
RR_AFSK_HD void afsk_lowpass(const AfskArgs& a, int tid, const float* TP, const float* D, float y[AFSK_R]) {
    const int L = a.g.L, Lc = L & ~7;
    int B = 8 * tid + L - 1 + a.g.padD;       // a multiple of 8; e[8 + k] = D[B + k], e[k] = D[B - 8 + k]
    float e[16], acc[AFSK_R];
    {
        const int b0 = afsk_sk(B - 8), b1 = afsk_sk(B);
#pragma unroll
        for (int k = 0; k < 8; k++) { e[k] = D[b0 + k]; e[8 + k] = D[b1 + k]; }
    }
#pragma unroll
    for (int r = 0; r < AFSK_R; r++) acc[r] = 0.0f;
    for (int j = 0; j < Lc; j += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const float t = TP[j + u];
#pragma unroll
            for (int r = 0; r < AFSK_R; r++) acc[r] = AFSK_FMA(t, e[8 + r - u], acc[r]);
        }
        B -= 8;
        const int nb = afsk_sk(B - 8);        // >= 7 floats into the front pad at the last chunk
#pragma unroll
        for (int k = 0; k < 8; k++) { e[8 + k] = e[k]; e[k] = D[nb + k]; }
    }
#pragma unroll
    for (int u = 0; u < 7; u++) {
        if (u < L - Lc) {
            const float t = TP[Lc + u];
#pragma unroll
            for (int r = 0; r < AFSK_R; r++) acc[r] = AFSK_FMA(t, e[8 + r - u], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < AFSK_R; r++) y[r] = AFSK_ADD(acc[r], a.offset);
}

}  // namespace rr
