// fsk_host.hpp — the host-only side of rr_fsk_tx: the refusals of create and push, the state of the two resamplers at any stream
// position (128-bit, for the tests), and a host twin of the handle that runs fsk_core.hpp's arithmetic one sample after the other
// (tests/cpp/emu_fsk.cpp builds it with the host sanitizers).  No HIP in here.
#pragma once
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

#include "fsk_core.hpp"

namespace rr {

enum { FSK_DIRECT = 0, FSK_AFSK = 1 };        // RR_FSK_TX_DIRECT, RR_FSK_TX_AFSK

// What rr_fsk_tx_create refuses, said before any device is touched; nullptr: fine.  k2 is not looked at in DIRECT mode.
inline const char* fsk_check(int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain, size_t interp2,
                             size_t deci2, double k2) {
    if (mode != FSK_DIRECT && mode != FSK_AFSK) return "fsk tx: unknown mode";
    if (!interp1 || !deci1 || !interp2 || !deci2) return "interpolation and decimation must be nonzero";     // rational_resampler.rs: Err
    for (size_t pair : {(size_t)0, (size_t)1}) {
        const size_t i = pair ? interp2 : interp1, d = pair ? deci2 : deci1;
        if (i > ((size_t)1 << 62) || d > ((size_t)1 << 62)) return "fsk tx: reduced ratio part above 2^31";
        const FskRatio r = fsk_ratio((long)i, (long)d);
        if (r.I > FSK_MAX_PART || r.D > FSK_MAX_PART) return "fsk tx: reduced ratio part above 2^31";
    }
    if (!std::isfinite(lo) || !std::isfinite(hi)) return "fsk tx: lo and hi must be finite";
    if (!std::isfinite(gain)) return "fsk tx: gain must be finite";
    if (!std::isfinite(k1) || (mode == FSK_AFSK && !std::isfinite(k2))) return "fsk tx: k1 and k2 must be finite";
    return nullptr;
}
// What a push refuses (nothing may be launched then); nullptr: fine, and *plan is the push.
inline const char* fsk_check_push(int mode, const FskPos& pos, const FskRatio& r1, const FskRatio& r2, const void* bits, size_t n_bits,
                                  const void* out, size_t out_cap, const void* audio, size_t audio_cap, FskPush* plan) {
    if (mode == FSK_DIRECT && audio) return "fsk tx: DIRECT mode has no audio output";
    if (n_bits > FSK_MAX_PUSH) return "fsk tx: more than 2^30 bits in one push";
    const FskPush u = fsk_plan(pos, r1, r2, (long)n_bits);
    if (u.no < 0) return "fsk tx: more than 2^30 audio samples in one push";
    if ((unsigned long long)u.no > FSK_MAX_PUSH) return "fsk tx: more than 2^30 outputs in one push";
    if (u.next.out > FSK_MAX_POS) return "fsk tx: output position beyond 2^62";
    if (n_bits && !bits) return "fsk tx: null bit buffer";
    if (u.no && !out) return "fsk tx: null output buffer";
    if (out_cap < (size_t)u.no) return "fsk tx: out_cap below the outputs of this push";
    if (audio && audio_cap < (size_t)u.na) return "fsk tx: audio_cap below the audio samples of this push";
    if (plan) *plan = u;
    return nullptr;
}

// The resamplers after `bits` inputs, from nothing but that number: A = ceil(bits I1 / D1), O = ceil(A I2 / D2) and the two
// residues, in 128-bit arithmetic.  The handle never needs it (it carries FskPos from push to push); the tests compare the two.
inline FskPos fsk_seek(const FskRatio& r1, const FskRatio& r2, unsigned long long bits) {
    typedef unsigned __int128 u128;
    FskPos p;
    p.bits = bits;
    const u128 a = ((u128)bits * (u128)r1.I + (u128)(r1.D - 1)) / (u128)r1.D;
    p.e1 = (long)(a * (u128)r1.D - (u128)bits * (u128)r1.I);
    const u128 o = (a * (u128)r2.I + (u128)(r2.D - 1)) / (u128)r2.D;
    p.e2 = (long)(o * (u128)r2.D - a * (u128)r2.I);
    p.audio = (unsigned long long)a;
    p.out = (unsigned long long)o;
    return p;
}

// The handle on the host, one sample after the other: the kernels' formulas with every scan sequential.  A tile of the device
// starts its sums anew, this does not: the two differ by roundings, both inside the bound.
struct FskHost {
    int mode;
    FskRatio r1, r2;
    float lo, hi, gain;
    double k1, k2, dhi, dlo;
    FskPos pos;
    double p1 = 0.0, p2 = 0.0;
    FskHost(int md, size_t i1, size_t d1, float l, float h, double kk1, float g, size_t i2, size_t d2, double kk2)
        : mode(md), r1(fsk_ratio((long)i1, (long)d1)), r2(fsk_ratio((long)i2, (long)d2)), lo(l), hi(h), gain(g), k1(kk1), k2(kk2),
          dhi(kk1 * (double)h), dlo(kk1 * (double)l) {}
    // -> the push; out and audio grow by what it made.  A push that is refused changes nothing and throws its sentence.
    FskPush push(const unsigned char* bits, size_t n, std::vector<std::complex<float>>& out, std::vector<float>* audio) {
        FskPush u{};
        static const char dummy = 0;
        if (const char* e = fsk_check_push(mode, pos, r1, r2, bits, n, &dummy, (size_t)-1, nullptr, 0, &u)) throw e;
        long c1 = 0;
        double base2 = p2, ph = p1;
        for (long m = 0; m < u.na; m++) {
            c1 += bits[fsk_src(r1, u.e1, m)] != 0;
            ph = fsk_phase1(p1, c1, m + 1 - c1, dhi, dlo);
            const float sn = (float)std::sin(ph), cs = (float)std::cos(ph);
            const long o0 = fsk_first(r2, u.e2, m), rep = fsk_first(r2, u.e2, m + 1) - o0;
            if (mode == FSK_DIRECT) {
                for (long j = 0; j < rep; j++) out.push_back({sn * gain, cs * gain});
                continue;
            }
            const float a = sn * gain;
            if (audio) audio->push_back(a);
            const double d = fsk_step(k2, a);
            for (long j = 1; j <= rep; j++) {
                const double q = fsk_wrap(base2 + fsk_red(j, d));
                out.push_back({(float)std::sin(q), (float)std::cos(q)});
            }
            base2 = fsk_wrap(base2 + fsk_wrap(fsk_red(rep, d)));
        }
        if (u.na) { p1 = ph; p2 = base2; }
        pos = u.next;
        return u;
    }
};

}  // namespace rr
