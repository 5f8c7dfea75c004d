// fsk_core.hpp — the index arithmetic of rr_fsk_tx and rr_fsk_tx_multi (kernels_tx.hip) shared by kernels and
// host: plain functions, no HIP types, so tests/cpp/test_fsk_hostlogic.cpp, emu_fsk.cpp and emu_fsk_multi.cpp compile them with g++.
//
// A RationalResampler (rational_resampler.rs:183-198) with the reduced ratio I : D is out[m] = in[floor(m D / I)] and has made
// ceil(N I / D) outputs after N inputs.  Input i owns the outputs [first(i), first(i + 1)), first(i) = ceil(i I / D), and
// rep(i) = first(i + 1) - first(i) of them.  Stream positions grow without bound and m * D leaves 64 bits long before they do, so
// nothing here multiplies a stream position: a push carries the residue
//   e = P_out * D - P_in * I,  0 <= e < D          (P_in inputs taken so far, P_out = ceil(P_in I / D) outputs made)
// and everything else is relative to the push:
//   first(i) = ceil((i I - e) / D)      src(m) = floor((e + m D) / I)      made(n) = first(n)
// With i, m <= 2^30 and I, D <= 2^31 every product stays below 2^61.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#define RR_FSK_HD __host__ __device__ __forceinline__
#else
#define RR_FSK_HD inline
#endif

namespace rr {

constexpr int FSK_T = 2048;                   // audio samples of one scan tile, 8 consecutive ones per thread
constexpr int FSK_OT = 2048;                  // outputs of one tile of the map kernel, 8 per thread, 256 apart
constexpr int FSK_B = 256;                    // threads of a workgroup
constexpr int FSK_PER = 8;
constexpr int FSK_SCAN_CHUNK = 4096;          // audio tiles one pass of the two tile-level scans takes (kernels_tx.hip VCO_SCHUNK)
constexpr long FSK_MAX_PART = 1L << 31;       // the largest part of a reduced ratio
constexpr unsigned long long FSK_MAX_PUSH = 1ull << 30;   // bits, audio samples and outputs of one push, each
constexpr unsigned long long FSK_MAX_POS = 1ull << 62;    // the output position a push may reach

struct FskRatio {
    long I, D;                                // reduced
    long qs, rs;                              // D / I, D % I: what src() moves by per output
    long qf, rf;                              // I / D, I % D: what first() moves by per input
};
RR_FSK_HD long fsk_gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }
RR_FSK_HD FskRatio fsk_ratio(long interp, long deci) {
    const long g = fsk_gcd(interp, deci);
    FskRatio r{};
    r.I = interp / g; r.D = deci / g;
    r.qs = r.D / r.I; r.rs = r.D % r.I;
    r.qf = r.I / r.D; r.rf = r.I % r.D;
    return r;
}
// the first output of input i of the push; i = n: the outputs the push makes.  i I - e > -D, so the numerator below is >= 0
RR_FSK_HD long fsk_first(const FskRatio& r, long e, long i) { return (i * r.I - e + r.D - 1) / r.D; }
RR_FSK_HD long fsk_rep(const FskRatio& r, long e, long i) { return fsk_first(r, e, i + 1) - fsk_first(r, e, i); }
// the input behind output m of the push
RR_FSK_HD long fsk_src(const FskRatio& r, long e, long m) { return (e + m * r.D) / r.I; }
// the residue behind a push of n inputs that made `made` outputs
RR_FSK_HD long fsk_next_e(const FskRatio& r, long e, long n, long made) { return e + made * r.D - n * r.I; }

// floor((x0 + t * step) / den) for t = 0, 1, 2, ... with one division: q and the remainder r move by step / den and step % den
struct FskWalk {
    long q, r, dq, dr, den;
    RR_FSK_HD void next() { q += dq; r += dr; if (r >= den) { r -= den; q += 1; } }
};
RR_FSK_HD FskWalk fsk_walk(long x0, long dq, long dr, long den) { return FskWalk{x0 / den, x0 % den, dq, dr, den}; }
// ... src(m0), src(m0 + 1), ...
RR_FSK_HD FskWalk fsk_walk_src(const FskRatio& r, long e, long m0) { return fsk_walk(e + m0 * r.D, r.qs, r.rs, r.I); }
// ... first(i0), first(i0 + 1), ...
RR_FSK_HD FskWalk fsk_walk_first(const FskRatio& r, long e, long i0) { return fsk_walk(i0 * r.I - e + r.D - 1, r.qf, r.rf, r.D); }

// Where the two resamplers stand between pushes.  Positions are kept for the 2^62 refusal and for rr_fsk_tx_count only.
struct FskPos {
    unsigned long long bits = 0, audio = 0, out = 0;
    long e1 = 0, e2 = 0;
};
// What a push of n bits from `p` is: na audio samples and no outputs (both may be 0), and where it leaves the resamplers.
struct FskPush {
    long n, na, no;
    long e1, e2;                              // the residues the push starts from
    FskPos next;
};
// n <= 2^30.  Audio beyond 2^30 samples is not multiplied further: no = -1 then, and the push is refused (fsk_host.hpp).
RR_FSK_HD FskPush fsk_plan(const FskPos& p, const FskRatio& r1, const FskRatio& r2, long n) {
    FskPush u{};
    u.n = n; u.e1 = p.e1; u.e2 = p.e2;
    u.na = fsk_first(r1, p.e1, n);
    if ((unsigned long long)u.na > FSK_MAX_PUSH) { u.no = -1; return u; }
    u.no = fsk_first(r2, p.e2, u.na);
    u.next.bits = p.bits + (unsigned long long)n;
    u.next.audio = p.audio + (unsigned long long)u.na;
    u.next.out = p.out + (unsigned long long)u.no;
    u.next.e1 = fsk_next_e(r1, p.e1, n, u.na);
    u.next.e2 = fsk_next_e(r2, p.e2, u.na, u.no);
    return u;
}
// What one stream of rr_fsk_tx_multi carries between pushes, all of it on the device: where its two resamplers
// stand and the two phases behind its last sample.  All zero at the start, as FskTx's FskPos and phases are.
struct FskStream {
    FskPos pos;
    double ph[2];                             // phase 1, phase 2
};
// ---- the phase arithmetic (DESIGN.md 4.20 has the error account) -------------------------------------------------------------
constexpr double FSK_MX = 2.0 * 3.14159265358979323846;   // vco.rs: 2.0 * f64::consts::PI

// vco.rs:27-32: |p| <= 2 MX in, |p| <= MX out, exact (kernels_tx.hip vco_wrap)
RR_FSK_HD double fsk_wrap(double p) {
    if (p > FSK_MX) p -= FSK_MX;
    if (p < -FSK_MX) p += FSK_MX;
    return p;
}
// one sample's increment k * a into [-MX, MX] (kernels_tx.hip vco_step)
RR_FSK_HD double fsk_step(double k, float a) {
    double d = k * (double)a;
    if (__builtin_fabs(d) > 2.0 * FSK_MX) d = __builtin_fma(-FSK_MX, __builtin_trunc(d * (1.0 / FSK_MX)), d);
    return fsk_wrap(d);
}
// c * d modulo MX into [-MX / 2, MX / 2] (a hair more where c * d is huge), c a count: the product enters as its rounded value p
// AND the exact rest fma(c, d, -p), whole turns leave p inside one fma, so the result is within 2^-51 of c * d - turns * MX
// whatever c is.  0 for c == 0.
RR_FSK_HD double fsk_red(long c, double d) {
    const double cd = (double)c;              // exact: c <= 2^31
    const double p = cd * d;
    const double rest = __builtin_fma(cd, d, -p);
    const double r = __builtin_fma(-FSK_MX, __builtin_rint(p * (1.0 / FSK_MX)), p);
    return r + rest;
}
// stage 1: the phase of the audio sample that has c1 one-samples and c0 zero-samples of the push up to and including itself,
// on top of the phase carried in; dhi = k1 * hi, dlo = k1 * lo in f64.  |result| <= MX.
RR_FSK_HD double fsk_phase1(double carried, long c1, long c0, double dhi, double dlo) {
    return fsk_wrap(carried + (fsk_red(c1, dhi) + fsk_red(c0, dlo)));
}

}  // namespace rr
