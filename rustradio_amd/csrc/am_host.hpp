// am_host.hpp — the host-only side of rr_am_demod: the refusals of create and push, the geometry of a push, and a host twin of
// the handle that takes am_core.hpp tile by tile and thread by thread with the kernel's indexing (tests/cpp/emu_am.cpp builds it
// with the host sanitizers).  No HIP in here.
#pragma once
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

#include "am_core.hpp"

namespace rr {

constexpr size_t AM_MAX_STREAMS = 4096;                   // the bound of rr_channelizer_create
constexpr size_t AM_MAX_PUSH = (size_t)1 << 30;           // nstreams * n and nstreams * produced of one push
constexpr size_t AM_MAX_RATIO = (size_t)1 << 31;          // interp and deci after the reduction

// What rr_am_demod_create refuses, said before any device is touched; nullptr: fine.
inline const char* am_check(size_t nstreams, const float* taps, size_t ntaps, size_t interp, size_t deci, float scale) {
    if (nstreams < 1 || nstreams > AM_MAX_STREAMS) return "nstreams out of range";
    if (!taps || ntaps < 1 || ntaps > (size_t)AM_MAX_TAPS) return "AmDemod needs 1 to 16384 finite taps";
    for (size_t i = 0; i < ntaps; i++)
        if (!std::isfinite(taps[i])) return "AmDemod needs 1 to 16384 finite taps";
    if (deci == 0) return "RationalResampler created using deci 0";                     // rational_resampler.rs
    if (interp == 0) return "RationalResampler created using interp 0";
    const size_t g = std::gcd(interp, deci);
    if (interp / g > AM_MAX_RATIO || deci / g > AM_MAX_RATIO) return "am demod: reduced ratio part above 2^31";
    if (!std::isfinite(scale)) return "scale must be finite";
    return nullptr;
}
inline AmGeom am_geom_of(size_t ntaps, size_t interp, size_t deci) {
    if (!ntaps || !interp || !deci) return AmGeom{};      // (am_check refuses these)
    const size_t g = std::gcd(interp, deci);
    return am_geom((int)ntaps, (long)(interp / g), (long)(deci / g));
}
// What a push refuses (nothing may be launched then); nullptr: fine.  e: where the handle stands (am_core.hpp).  *produced is
// written whenever the lengths are in range.
inline const char* am_check_push(size_t nstreams, const AmGeom& g, long e, const void* in, size_t in_stride, size_t n, const void* out,
                                 size_t out_stride, size_t* produced) {
    *produced = 0;
    if (n > AM_MAX_PUSH || nstreams * n > AM_MAX_PUSH) return "am demod: more than 2^30 samples in one push";
    const size_t k = (size_t)am_produced(e, (long)n, g.I, g.D);
    if (k > AM_MAX_PUSH || nstreams * k > AM_MAX_PUSH) return "am demod: more than 2^30 outputs in one push";
    if (in_stride < n) return "am demod: in_stride below n";
    if (out_stride < k) return "am demod: out_stride below produced";
    if ((n && !in) || (k && !out)) return "am demod: null buffer";
    *produced = k;
    return nullptr;
}
// Elements from the first stream's first to the last stream's last: what a host push moves in one piece.  0 for n == 0.
inline size_t am_span_elems(size_t nstreams, size_t stride, size_t n) { return n ? (nstreams - 1) * stride + n : 0; }

// The handle on the host: the same carry pair, the same plan, every tile of the grid with every thread of its workgroup in turn.
struct AmHost {
    size_t nstreams;
    AmGeom g;
    std::vector<float> taps, carry[2];
    int cur = 0;
    long e = 0;                                           // where every stream stands
    unsigned long long total = 0;                         // samples every stream has taken
    float scale;
    AmHost(size_t ns, const std::vector<float>& tp, size_t interp, size_t deci, float sc)
        : nstreams(ns), g(am_geom_of(tp.size(), interp, deci)), taps(tp), scale(sc) {
        if (const char* err = am_check(ns, tp.data(), tp.size(), interp, deci, sc)) throw err;
        for (auto& c : carry) c.assign(ns * (size_t)g.C + 1, 0.0f);
    }
    // in: (re, im) pairs -> produced (the same for every stream); a push that is refused changes nothing and throws its sentence
    size_t push(const float* in, size_t in_stride, size_t n, float* out, size_t out_stride) {
        size_t produced = 0;
        if (const char* err = am_check_push(nstreams, g, e, in, in_stride, n, out, out_stride, &produced)) throw err;
        if (!n) return 0;
        AmArgs a{};
        a.g = g;
        a.in = in; a.in_stride = (long)in_stride; a.n = (long)n;
        a.out = out; a.out_stride = (long)out_stride; a.produced = (long)produced;
        a.carry_in = carry[cur].data(); a.carry_out = carry[cur ^ 1].data();
        a.taps = taps.data();
        a.scale = scale;
        a.e = e;
        const long ntiles = am_tiles(g, a.produced);
        std::vector<float> S((size_t)AM_LDS_FLOATS);
        std::vector<int> B((size_t)g.T);
        std::vector<float> acc((size_t)AM_NT * AM_NG_MAX * AM_G);
        for (long c = 0; c < (long)nstreams; c++)
            for (long tx = 0; tx < ntiles; tx++) {
                if (tx == ntiles - 1)
                    for (int t = 0; t < AM_NT; t++) am_carry(a, c, t);
                const int nk = am_tile_nk(a, tx);
                if (!nk) continue;
                for (int t = 0; t < g.T; t++) B[(size_t)t] = am_base(a, tx, t < nk ? t : nk - 1);
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int j0 = 0; j0 < g.L; j0 += g.KC) {
                    for (int t = 0; t < AM_NT; t++) am_stage(a, c, tx, nk, j0, t, S.data());
                    for (int t = 0; t < AM_NT; t++) {
                        const int lane = t & 63, w = t >> 6;
                        for (int gi = 0; gi < g.NG; gi++) {
                            const int r0 = (AM_WAVES * gi + w) * AM_G;
                            if (r0 >= nk) continue;
                            am_accum(a, j0, lane, &B[(size_t)r0], S.data(), &acc[((size_t)t * AM_NG_MAX + (size_t)gi) * AM_G]);
                        }
                    }
                }
                for (int w = 0; w < AM_WAVES; w++)
                    for (int gi = 0; gi < g.NG; gi++) {
                        const int r0 = (AM_WAVES * gi + w) * AM_G;
                        for (int u = 0; u < AM_G && r0 + u < nk; u++) {
                            float v[64];
                            for (int l = 0; l < 64; l++) v[l] = acc[((size_t)(64 * w + l) * AM_NG_MAX + (size_t)gi) * AM_G + (size_t)u];
                            out[(size_t)c * out_stride + (size_t)(tx * g.T + r0 + u)] = am_scale(a, am_tree(v));
                        }
                    }
            }
        cur ^= 1;
        e = am_next_e(e, (long)n, a.produced, g.I, g.D);
        total += n;
        return produced;
    }
};

}  // namespace rr
