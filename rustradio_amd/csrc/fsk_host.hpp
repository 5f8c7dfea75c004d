// fsk_host.hpp — the host-only side of rr_fsk_tx: the refusals of create and push, the state of the two resamplers at any stream
// position (128-bit, for the tests), and a host twin of the handle that runs fsk_core.hpp's arithmetic one sample after the other
// (tests/cpp/emu_fsk.cpp builds it with the host sanitizers); and the same for rr_fsk_tx_multi: its refusals, the bound of a push
// and the twin FskMultiHost (tests/cpp/emu_fsk_multi.cpp).  No HIP in here.
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

// ---- rr_fsk_tx_multi: nstreams streams behind one handle, every stream's FskPos on the device -------------------
constexpr size_t FSK_MAX_STREAMS = 65535;     // the grid's y, as rr_afsk_demod has it

// What rr_fsk_tx_multi_create refuses, said before any device is touched: fsk_check's, then the stream count.
inline const char* fsk_multi_check(size_t nstreams, int mode, size_t interp1, size_t deci1, float lo, float hi, double k1, float gain,
                                   size_t interp2, size_t deci2, double k2) {
    if (const char* e = fsk_check(mode, interp1, deci1, lo, hi, k1, gain, interp2, deci2, k2)) return e;
    if (!nstreams || nstreams > FSK_MAX_STREAMS) return "nstreams out of range";
    return nullptr;
}
// ceil(x I / D), saturated at the largest size_t
inline size_t fsk_made_sat(size_t x, const FskRatio& r) {
    typedef unsigned __int128 u128;
    const u128 v = ((u128)x * (u128)r.I + (u128)(r.D - 1)) / (u128)r.D;
    return v > (u128)(size_t)-1 ? (size_t)-1 : (size_t)v;
}
// The most one stream can make from n_cap bits whatever its residues: first(n) = ceil((n I - e) / D) is largest at e = 0, so
// audio_cap = ceil(n_cap I1 / D1) and out_cap = ceil(audio_cap I2 / D2).  Strides, scratch and grids are sized from these.
inline void fsk_multi_bound(const FskRatio& r1, const FskRatio& r2, size_t n_cap, size_t* audio_cap, size_t* out_cap) {
    *audio_cap = fsk_made_sat(n_cap, r1);
    *out_cap = fsk_made_sat(*audio_cap, r2);
}
// What a push refuses (nothing may be launched then); nullptr: fine, and *audio_cap / *out_cap are the bound of the push.  The
// host cannot know the device's positions: bits_bound, the sum of the n_cap of all pushes so far, is above every stream's.
inline const char* fsk_multi_check_push(int mode, size_t nstreams, const FskRatio& r1, const FskRatio& r2, unsigned long long bits_bound,
                                        const void* bits, size_t bits_stride, size_t n_cap, const void* out, size_t out_stride,
                                        const void* audio, size_t audio_stride, size_t* audio_cap, size_t* out_cap) {
    if (mode == FSK_DIRECT && audio) return "fsk tx multi: DIRECT mode has no audio output";
    if (n_cap > FSK_MAX_PUSH) return "fsk tx multi: more than 2^30 bits of a stream in one push";
    size_t ac = 0, oc = 0;
    fsk_multi_bound(r1, r2, n_cap, &ac, &oc);
    if (ac > FSK_MAX_PUSH / nstreams) return "fsk tx multi: more than 2^30 audio samples of all streams in one push";
    if (oc > FSK_MAX_PUSH / nstreams) return "fsk tx multi: more than 2^30 outputs of all streams in one push";
    if (bits_bound > (1ull << 63) || fsk_made_sat(fsk_made_sat((size_t)bits_bound + n_cap, r1), r2) > FSK_MAX_POS)
        return "fsk tx multi: output position beyond 2^62";
    if (bits_stride < n_cap) return "fsk tx multi: bits_stride below n_cap";
    if (out_stride < oc) return "fsk tx multi: out_stride below the outputs a stream can make";
    if (audio && audio_stride < ac) return "fsk tx multi: audio_stride below the audio samples a stream can make";
    if (n_cap && !bits) return "fsk tx multi: null bit buffer";
    if (oc && !out) return "fsk tx multi: null output buffer";
    if (audio_cap) *audio_cap = ac;
    if (out_cap) *out_cap = oc;
    return nullptr;
}
// What the device says a stream made in a push, checked against the bound before anybody uses it
inline const char* fsk_multi_check_counts(const unsigned long long* made, size_t nstreams, size_t audio_cap, size_t out_cap) {
    for (size_t c = 0; c < nstreams; c++)
        if (made[c] > audio_cap || made[nstreams + c] > out_cap) return "fsk tx multi: the device's counts exceed the bound of the push";
    return nullptr;
}

// The handle on the host: nstreams FskHosts and the clamp of the counts, one stream after the other.
struct FskMultiHost {
    std::vector<FskHost> s;
    FskMultiHost(size_t nstreams, int md, size_t i1, size_t d1, float l, float h, double kk1, float g, size_t i2, size_t d2, double kk2)
        : s(nstreams, FskHost(md, i1, d1, l, h, kk1, g, i2, d2, kk2)) {}
    // stream c takes the next min(counts[c], n_cap) bits at bits + c * bits_stride (counts == nullptr: n_cap each); out[c] and
    // (*audio)[c] grow by what it made -> the pushes
    std::vector<FskPush> push(const unsigned char* bits, size_t bits_stride, size_t n_cap, const unsigned long long* counts,
                              std::vector<std::vector<std::complex<float>>>& out, std::vector<std::vector<float>>* audio) {
        std::vector<FskPush> u(s.size());
        for (size_t c = 0; c < s.size(); c++) {
            const size_t n = counts && counts[c] < n_cap ? (size_t)counts[c] : n_cap;
            u[c] = s[c].push(bits + c * bits_stride, n, out[c], audio ? &(*audio)[c] : nullptr);
        }
        return u;
    }
};

}  // namespace rr
