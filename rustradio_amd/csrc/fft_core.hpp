// fft_core.hpp — register-resident radix-2/4/8/16 butterflies and the in-place
// mixed-radix pass geometry used by the FftFilter kernels (kernels_fft.hip).
//
// Design (MI355X-first, not a translation of rustfft): one workgroup of F/16
// threads owns one F-point tile; every thread keeps 16 complex values in VGPRs.
// The forward transform is an in-place decimation-in-frequency mixed-radix FFT
// whose output is left in digit-reversed order; the frequency response H is
// stored in that same order, and the inverse transform is the exact mirror
// (decimation-in-time, digit-reversed in -> natural out).  That removes every
// reordering pass: data only crosses LDS where the next radix group needs
// values held by other lanes.
//
// Everything here is __host__ __device__ so tests/cpu_emulate_fft.cpp can run the
// same pass functions thread-by-thread on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RR_HD __host__ __device__ __forceinline__
#else
#define RR_HD inline
#endif

namespace rr {

struct alignas(8) cf { float x, y; };   // Complex<f32>, interleaved (src/lib.rs:268-271)
RR_HD cf mkcf(float x, float y) { cf r; r.x = x; r.y = y; return r; }

// evaluated in double, rounded once
constexpr float kSqrtHalf = (float)0.70710678118654752440;
constexpr float kCos8 = (float)0.92387953251128675613;   // cos(pi/8)
constexpr float kSin8 = (float)0.38268343236508977173;   // sin(pi/8)
constexpr float kTan8 = (float)0.41421356237309504880;   // tan(pi/8)  = sin(pi/8) / cos(pi/8)
constexpr float kCot8 = (float)2.41421356237309504880;   // tan(3pi/8) = cos(pi/8) / sin(pi/8)

// The butterflies' real constants, named by their slot: two share one SGPR pair on the device (op_sel picks the half), so
// that the five take three pairs.  The persistent-register kernels have no SGPR to spare.
enum { K_TAN8, K_COT8, K_COS8, K_SIN8, K_SQRT_HALF };
template <int K> constexpr float kval() { return K == K_TAN8 ? kTan8 : K == K_COT8 ? kCot8 : K == K_COS8 ? kCos8 : K == K_SIN8 ? kSin8 : kSqrtHalf; }

// Register type of the transform.  On the device a complex value lives in an aligned VGPR
// pair (ext_vector float2) so that complex add/sub are single v_pk_add_f32 and a complex
// multiply is v_pk_mul_f32 + v_pk_fma_f32: the +-j rotations and the (-im, re) swizzle of
// the multiply ride on the VOP3P op_sel / neg modifiers instead of costing instructions.
// hipcc only emits those modifiers for splats and negation, so the swizzled forms are
// written as (non-volatile, register-only) inline asm.  On the host (CPU emulation test)
// the same functions are plain C++.
#if defined(__HIP_DEVICE_COMPILE__)
typedef float creg __attribute__((ext_vector_type(2)));
RR_HD creg mk(float x, float y) { creg r; r.x = x; r.y = y; return r; }
RR_HD creg cadd(creg a, creg b) { return a + b; }
RR_HD creg csub(creg a, creg b) { return a - b; }
// a + (-j) b = (a.x + b.y, a.y - b.x)
RR_HD creg add_mj(creg a, creg b) {
    creg r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + (+j) b = (a.x - b.y, a.y + b.x)
RR_HD creg add_pj(creg a, creg b) {
    creg r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a * w = a * w.xx + (-a.y, a.x) * w.yy
RR_HD creg cmul(creg a, creg w) {
    creg t = a * __builtin_shufflevector(w, w, 0, 0), r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]"
        : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// a * conj(w) = a * w.xx + (a.y, -a.x) * w.yy
RR_HD creg cmulc(creg a, creg w) {
    creg t = a * __builtin_shufflevector(w, w, 0, 0), r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]"
        : "=v"(r) : "v"(a), "v"(w), "v"(t));
    return r;
}
// Two independent products issued interleaved (mul, mul, fma, fma): a packed FMA that reads the result of the packed
// multiply right before it costs a wait state (hipcc puts an s_nop between them — 88 of the 787 issue slots of a 2048-point
// tile); with the partner's multiply in between there is nothing to wait for.
RR_HD void cmul2(creg& a0, creg w0, creg& a1, creg w1) {
    creg t0 = a0 * __builtin_shufflevector(w0, w0, 0, 0);
    creg t1 = a1 * __builtin_shufflevector(w1, w1, 0, 0);
    creg r0, r1;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(r0) : "v"(a0), "v"(w0), "v"(t0));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(r1) : "v"(a1), "v"(w1), "v"(t1));
    a0 = r0; a1 = r1;
}
RR_HD void cmulc2(creg& a0, creg w0, creg& a1, creg w1) {
    creg t0 = a0 * __builtin_shufflevector(w0, w0, 0, 0);
    creg t1 = a1 * __builtin_shufflevector(w1, w1, 0, 0);
    creg r0, r1;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]" : "=v"(r0) : "v"(a0), "v"(w0), "v"(t0));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]" : "=v"(r1) : "v"(a1), "v"(w1), "v"(t1));
    a0 = r0; a1 = r1;
}
// Constant K's SGPR pair, (kval<K & ~1>, kval<K | 1>): an "s" operand is one constant-bus read, where VGPRs would be hoisted
// out of the tile loop and kept for the whole kernel
template <int K> RR_HD creg kpair() { return mk(kval<(K & ~1)>(), kval<(K | 1) <= K_SQRT_HALF ? (K | 1) : K>()); }
// a + k u and a - k u, k = kval<K>: ONE packed FMA (hipcc emits the splat of an SGPR by itself), the minus on u's neg
// modifier so that -k takes no SGPR of its own.  Written as asm these two cost 9 more s_nop per 2048-point tile.
template <int K> RR_HD creg fma_k(creg u, creg a) { return __builtin_elementwise_fma(u, mk(kval<K>(), kval<K>()), a); }
template <int K> RR_HD creg fms_k(creg u, creg a) { return __builtin_elementwise_fma(-u, mk(kval<K>(), kval<K>()), a); }
// a + k (-j u) = (a.x + k u.y, a.y - k u.x) and a + k (+j u) = (a.x - k u.y, a.y + k u.x): the rotation rides on the
// modifiers as in add_mj / add_pj
template <int K> RR_HD creg fma_mj_k(creg u, creg a) {
    creg r;
    if constexpr (K & 1) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(u), "s"(kpair<K>()), "v"(a));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(u), "s"(kpair<K>()), "v"(a));
    return r;
}
template <int K> RR_HD creg fma_pj_k(creg u, creg a) {
    creg r;
    if constexpr (K & 1) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(u), "s"(kpair<K>()), "v"(a));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(u), "s"(kpair<K>()), "v"(a));
    return r;
}
RR_HD creg to_reg(cf a) { return mk(a.x, a.y); }
RR_HD cf from_reg(creg a) { cf r; r.x = a.x; r.y = a.y; return r; }
#else
typedef cf creg;
RR_HD creg mk(float x, float y) { cf r; r.x = x; r.y = y; return r; }
RR_HD creg cadd(creg a, creg b) { return mk(a.x + b.x, a.y + b.y); }
RR_HD creg csub(creg a, creg b) { return mk(a.x - b.x, a.y - b.y); }
RR_HD creg add_mj(creg a, creg b) { return mk(a.x + b.y, a.y - b.x); }
RR_HD creg add_pj(creg a, creg b) { return mk(a.x - b.y, a.y + b.x); }
RR_HD creg cmul(creg a, creg b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
RR_HD creg cmulc(creg a, creg b) { return mk(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
template <int K> RR_HD creg fma_k(creg u, creg a) { return mk(fmaf(kval<K>(), u.x, a.x), fmaf(kval<K>(), u.y, a.y)); }
template <int K> RR_HD creg fms_k(creg u, creg a) { return mk(fmaf(-kval<K>(), u.x, a.x), fmaf(-kval<K>(), u.y, a.y)); }
template <int K> RR_HD creg fma_mj_k(creg u, creg a) { return mk(fmaf(kval<K>(), u.y, a.x), fmaf(-kval<K>(), u.x, a.y)); }
template <int K> RR_HD creg fma_pj_k(creg u, creg a) { return mk(fmaf(-kval<K>(), u.y, a.x), fmaf(kval<K>(), u.x, a.y)); }
RR_HD void cmul2(creg& a0, creg w0, creg& a1, creg w1) { a0 = cmul(a0, w0); a1 = cmul(a1, w1); }
RR_HD void cmulc2(creg& a0, creg w0, creg& a1, creg w1) { a0 = cmulc(a0, w0); a1 = cmulc(a1, w1); }
RR_HD creg to_reg(cf a) { return a; }
RR_HD cf from_reg(creg a) { return a; }
#endif

// RR_LDS_Q = volatile keeps hipcc from fusing neighbouring 8-byte LDS accesses into
// ds_read2_b64 / ds_write2_b64 (a tuning experiment; see profiles/TUNING_LOG.md).
#ifndef RR_LDS_Q
#define RR_LDS_Q
#endif

// a + w4 b and a - w4 b, w4 = -j (forward) or +j (inverse): the rotation is free
template <bool INV> RR_HD creg add_w4(creg a, creg b) { return INV ? add_pj(a, b) : add_mj(a, b); }
template <bool INV> RR_HD creg sub_w4(creg a, creg b) { return INV ? add_mj(a, b) : add_pj(a, b); }
// a + k (w4 u) and a - k (w4 u), k = kval<K>: -w4 is the w4 of the other direction
template <bool INV, int K> RR_HD creg fma_w4_k(creg u, creg a) { return INV ? fma_pj_k<K>(u, a) : fma_mj_k<K>(u, a); }
template <bool INV, int K> RR_HD creg fms_w4_k(creg u, creg a) { return INV ? fma_mj_k<K>(u, a) : fma_pj_k<K>(u, a); }
// x + t (w4 x), t = kval<T>: the product w x without its real factor c, for w = c (1 -+ j t) = exp(-+ j atan t)
template <bool INV, int T> RR_HD creg rot_tan(creg x) { return fma_w4_k<INV, T>(x, x); }

// The constant rotations w16^m between the two layers of Dft<8> / Dft<16> cost no multiply of their own: each is
// written c (1 + t w4) (m = 1, 3, 9: t = tan, one rot_tan), (+-1 + w4) sqrt(1/2) (m = 2, 6: one add_w4 / sub_w4) or w4
// itself (m = 4: nothing), and the real factor c that is left rides on the FMAs of the butterfly that consumes the value.

template <bool INV> RR_HD void bfly2(creg& a, creg& b) {
    creg t = csub(a, b);
    a = cadd(a, b);
    b = t;
}

// natural-order 4-point DFT in place
template <bool INV> RR_HD void bfly4(creg& a0, creg& a1, creg& a2, creg& a3) {
    creg t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = csub(a1, a3);
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = add_w4<INV>(t1, t3);
    a3 = sub_w4<INV>(t1, t3);
}

// R-point DFT of v[0..R) (stride 1 in the register array), natural order in and out.
template <int R, bool INV> struct Dft;

template <bool INV> struct Dft<2, INV> {
    static RR_HD void run(creg* v) { bfly2<INV>(v[0], v[1]); }
};
template <bool INV> struct Dft<4, INV> {
    static RR_HD void run(creg* v) { bfly4<INV>(v[0], v[1], v[2], v[3]); }
};
// the second half of a 4-point DFT whose odd sums carry an outstanding real factor k = kval<K>:
// (a0, a2) = t0 +- k t2, (a1, a3) = t1 +- k (w4 t3)
template <bool INV, int K> RR_HD void bfly4_out_k(creg& a0, creg& a1, creg& a2, creg& a3, creg t0, creg t1, creg t2, creg t3) {
    a0 = fma_k<K>(t2, t0);
    a2 = fms_k<K>(t2, t0);
    a1 = fma_w4_k<INV, K>(t3, t1);
    a3 = fms_w4_k<INV, K>(t3, t1);
}
// natural-order 4-point DFT in place of (a0, k1 a1, +-k2 a2, +-kr k1 a3), minus with NEG: the real factors kval<K1>,
// kval<K2>, kval<KR> ride on the FMAs
template <bool INV, bool NEG, int K1, int K2, int KR> RR_HD void bfly4_k(creg& a0, creg& a1, creg& a2, creg& a3) {
    creg p0 = fma_k<K2>(a2, a0), m0 = fms_k<K2>(a2, a0), p1 = fma_k<KR>(a3, a1), m1 = fms_k<KR>(a3, a1);
    if constexpr (NEG) bfly4_out_k<INV, K1>(a0, a1, a2, a3, m0, p0, m1, p1);
    else bfly4_out_k<INV, K1>(a0, a1, a2, a3, p0, m0, p1, m1);
}

template <bool INV> struct Dft<8, INV> {
    // n = 2 n1 + n2 (N1 = 4, N2 = 2), k = k1 + 4 k2
    static RR_HD void run(creg* v) {
        bfly4<INV>(v[0], v[2], v[4], v[6]);
        bfly4<INV>(v[1], v[3], v[5], v[7]);
        // v[2 k1 + 1] *= w8^k1, folded into the 2-point butterflies
        creg u3 = add_w4<INV>(v[3], v[3]);   // w8^1 v[3] = sqrt(1/2) u3
        creg u7 = sub_w4<INV>(v[7], v[7]);   // w8^3 v[7] = -sqrt(1/2) u7
        bfly2<INV>(v[0], v[1]);
        v[3] = fms_k<K_SQRT_HALF>(u3, v[2]); v[2] = fma_k<K_SQRT_HALF>(u3, v[2]);
        creg t = sub_w4<INV>(v[4], v[5]);    // w8^2 = w4
        v[4] = add_w4<INV>(v[4], v[5]); v[5] = t;
        v[7] = fma_k<K_SQRT_HALF>(u7, v[6]); v[6] = fms_k<K_SQRT_HALF>(u7, v[6]);
        // v[2 k1 + k2] = X[k1 + 4 k2]  ->  natural order
        creg t1 = v[1], t2 = v[2], t3 = v[3], t4 = v[4], t5 = v[5], t6 = v[6];
        v[1] = t2; v[2] = t4; v[3] = t6; v[4] = t1; v[5] = t3; v[6] = t5;
    }
};
template <bool INV> struct Dft<16, INV> {
    // n = 4 n1 + n2, k = k1 + 4 k2
    static RR_HD void run(creg* v) {
        bfly4<INV>(v[0], v[4], v[8], v[12]);
        bfly4<INV>(v[1], v[5], v[9], v[13]);
        bfly4<INV>(v[2], v[6], v[10], v[14]);
        bfly4<INV>(v[3], v[7], v[11], v[15]);
        // v[4 k1 + n2] *= w16^(n2 k1), each without its real factor (in brackets); the three rows side by side, so that no
        // packed FMA reads the result of the one right before it (cmul2's wait state)
        v[5] = rot_tan<INV, K_TAN8>(v[5]);    // w16^1  [cos(pi/8)]
        v[13] = rot_tan<INV, K_COT8>(v[13]);  // w16^3  [sin(pi/8)]
        v[7] = rot_tan<INV, K_COT8>(v[7]);    // w16^3  [sin(pi/8)]
        v[15] = rot_tan<INV, K_TAN8>(v[15]);  // w16^9  [-cos(pi/8)]
        v[6] = add_w4<INV>(v[6], v[6]);      // w16^2  [sqrt(1/2)]
        v[14] = sub_w4<INV>(v[14], v[14]);   // w16^6  [-sqrt(1/2)]
        v[9] = add_w4<INV>(v[9], v[9]);      // w16^2  [sqrt(1/2)]
        v[11] = sub_w4<INV>(v[11], v[11]);   // w16^6  [-sqrt(1/2)]; w16^4 v[10] = w4 v[10] rides on row 2's first layer
        bfly4<INV>(v[0], v[1], v[2], v[3]);
        bfly4_k<INV, false, K_COS8, K_SQRT_HALF, K_TAN8>(v[4], v[5], v[6], v[7]);
        {   // row 2: the odd pair's factors are +- sqrt(1/2), so its sums are plain
            creg t0 = add_w4<INV>(v[8], v[10]), t1 = sub_w4<INV>(v[8], v[10]), t2 = csub(v[9], v[11]), t3 = cadd(v[9], v[11]);
            bfly4_out_k<INV, K_SQRT_HALF>(v[8], v[9], v[10], v[11], t0, t1, t2, t3);
        }
        bfly4_k<INV, true, K_SIN8, K_SQRT_HALF, K_COT8>(v[12], v[13], v[14], v[15]);
        // v[4 k1 + k2] = X[k1 + 4 k2]  -> transpose 4x4 to natural order
        creg t;
        t = v[1]; v[1] = v[4]; v[4] = t;
        t = v[2]; v[2] = v[8]; v[8] = t;
        t = v[3]; v[3] = v[12]; v[12] = t;
        t = v[6]; v[6] = v[9]; v[9] = t;
        t = v[7]; v[7] = v[13]; v[13] = t;
        t = v[11]; v[11] = v[14]; v[14] = t;
    }
};

// ---- pass geometry ----------------------------------------------------------------
// F = R1 * R2 * ... * Rm.  Index n = sum_i n_i * P_i with P_i = R_{i+1} ... R_m.
// Pass i transforms digit i in place (n_i -> k_i); output bin k = k1 + R1 k2 + R1 R2 k3 ...
// sits at position sum_i k_i P_i ("digit reversed").
template <int LOG2F> struct Plan;
template <> struct Plan<10> { static constexpr int NP = 3; static constexpr int R[4] = {16, 16, 4, 1}; };
template <> struct Plan<11> { static constexpr int NP = 3; static constexpr int R[4] = {16, 16, 8, 1}; };
template <> struct Plan<12> { static constexpr int NP = 3; static constexpr int R[4] = {16, 16, 16, 1}; };
template <> struct Plan<13> { static constexpr int NP = 4; static constexpr int R[4] = {16, 16, 16, 2}; };
template <> struct Plan<14> { static constexpr int NP = 4; static constexpr int R[4] = {16, 16, 16, 4}; };

template <int LOG2F, int I> struct PassGeom {
    using P_ = Plan<LOG2F>;
    static constexpr int F = 1 << LOG2F;
    static constexpr int T = F / 16;                 // threads per tile
    static constexpr int R = P_::R[I];
    static constexpr int U = 16 / R;                 // groups per thread
    static constexpr int prodAfter() { int p = 1; for (int l = I + 1; l < P_::NP; l++) p *= P_::R[l]; return p; }
    static constexpr int P = prodAfter();            // stride of digit I
    static constexpr int TWSTRIDE = F / (R * P);     // twiddle table step: w_{R P}^1 = w_F^TWSTRIDE
    // in-place position of element n of group g
    static RR_HD int pos(int g, int n) { return (g / P) * (R * P) + (g % P) + n * P; }
    static RR_HD int lo(int g) { return g % P; }
};

// position -> frequency bin for the digit-reversed layout
template <int LOG2F> RR_HD int bin_of_pos(int pos) {
    using P_ = Plan<LOG2F>;
    int Pi = 1 << LOG2F, k = 0, mul = 1;
    for (int i = 0; i < P_::NP; i++) {
        Pi /= P_::R[i];
        int d = (pos / Pi) % P_::R[i];
        k += d * mul;
        mul *= P_::R[i];
    }
    return k;
}

// LDS padding: one 8-byte slot per 16 elements (keeps stride-P and stride-R accesses
// conflict-free for ds_read_b64/ds_write_b64; see profiles/TUNING_LOG.md).
RR_HD int lds_pad(int a) { return a + (a >> 4); }
constexpr int lds_elems(int F) { return F + (F >> 4); }

// Per-thread twiddles of pass I: twl[k-1] = w_{R P}^{k lo} = tw[k * lo * TWSTRIDE], k = 1..15.
// Only radix-16 passes (one group per thread) carry twiddles in every Plan above.
template <int LOG2F, int I> RR_HD constexpr bool pass_has_twiddles() { return PassGeom<LOG2F, I>::P > 1; }
template <int LOG2F, int I> RR_HD void load_twiddles(creg* twl, int t, const cf* __restrict__ tw) {
    using G = PassGeom<LOG2F, I>;
    static_assert(G::P == 1 || G::U == 1, "twiddled passes must be radix 16");
    if constexpr (G::P > 1) {
        const int lo = G::lo(t);
#pragma unroll
        for (int k = 1; k < 16; k++) twl[k - 1] = to_reg(tw[k * lo * G::TWSTRIDE]);
    }
}
// One forward pass on the 16 registers of a thread.  `v[u*R + n]` = element n of group
// (t + T u); twl = this thread's twiddles for the pass (unused when P == 1).
template <int LOG2F, int I> RR_HD void fwd_pass(creg* v, const creg* twl) {
    using G = PassGeom<LOG2F, I>;
#pragma unroll
    for (int u = 0; u < G::U; u++) Dft<G::R, false>::run(v + u * G::R);
    if constexpr (G::P > 1) {
        v[1] = cmul(v[1], twl[0]);
#pragma unroll
        for (int k = 2; k < 16; k += 2) cmul2(v[k], twl[k - 1], v[k + 1], twl[k]);
    }
}
// Mirror: conj twiddle first, then inverse DFT of the digit.
template <int LOG2F, int I> RR_HD void inv_pass(creg* v, const creg* twl) {
    using G = PassGeom<LOG2F, I>;
    if constexpr (G::P > 1) {
        v[1] = cmulc(v[1], twl[0]);
#pragma unroll
        for (int k = 2; k < 16; k += 2) cmulc2(v[k], twl[k - 1], v[k + 1], twl[k]);
    }
#pragma unroll
    for (int u = 0; u < G::U; u++) Dft<G::R, true>::run(v + u * G::R);
}

// LDS addressing of a pass layout, split into ONE per-thread base and compile-time
// offsets so that every ds_read/ds_write uses base VGPR + immediate:
//   lds_pad(pos(t + T u, n)) == lds_base<I>(t) + lds_off<I>(u, n)
// (holds because every twiddled pass has U == 1 and every multi-group pass has P == 1,
//  and n*P never carries into bit 4 together with the group's low part; see profiles/TUNING_LOG.md).
template <int LOG2F, int I> RR_HD int lds_base(int t) {
    using G = PassGeom<LOG2F, I>;
    static_assert(G::U == 1 || G::P == 1, "plan shape");
    if constexpr (G::P == 1) return G::R * t + ((G::R * t) >> 4);
    else return lds_pad((t / G::P) * (G::R * G::P) + (t % G::P));
}
template <int LOG2F, int I> RR_HD constexpr int lds_off(int u, int n) {
    using G = PassGeom<LOG2F, I>;
    if (G::P == 1) return n + u * G::R * G::T + ((u * G::R * G::T) >> 4);
    return n * G::P + ((n * G::P) >> 4);
}
template <int LOG2F, int I> RR_HD void lds_store(const creg* v, int t, creg* lds) {
    using G = PassGeom<LOG2F, I>;
    RR_LDS_Q creg* b = lds + lds_base<LOG2F, I>(t);
#pragma unroll
    for (int u = 0; u < G::U; u++)
#pragma unroll
        for (int n = 0; n < G::R; n++) b[lds_off<LOG2F, I>(u, n)] = v[u * G::R + n];
}
template <int LOG2F, int I> RR_HD void lds_load(creg* v, int t, const creg* lds) {
    using G = PassGeom<LOG2F, I>;
    const RR_LDS_Q creg* b = lds + lds_base<LOG2F, I>(t);
#pragma unroll
    for (int u = 0; u < G::U; u++)
#pragma unroll
        for (int n = 0; n < G::R; n++) v[u * G::R + n] = b[lds_off<LOG2F, I>(u, n)];
}
// H in position order: this thread's 16 values for the layout of pass I
template <int LOG2F, int I> RR_HD void load_h(creg* h, int t, const cf* __restrict__ hpos) {
    using G = PassGeom<LOG2F, I>;
#pragma unroll
    for (int u = 0; u < G::U; u++)
#pragma unroll
        for (int n = 0; n < G::R; n++) h[u * G::R + n] = to_reg(hpos[G::pos(t + G::T * u, n)]);
}
RR_HD void apply_h(creg* v, const creg* h) {
#pragma unroll
    for (int n = 0; n < 16; n += 2) cmul2(v[n], h[n], v[n + 1], h[n + 1]);
}

}  // namespace rr
