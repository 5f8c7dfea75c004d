// afsk_host.hpp — the host-only side of rr_afsk_demod: the refusals of create and push, the geometry of a push, and a host twin
// of the handle that takes afsk_core.hpp tile by tile and thread by thread with the kernel's indexing (tests/cpp/emu_afsk.cpp
// builds it with the host sanitizers).  No HIP in here.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "afsk_core.hpp"

namespace rr {

constexpr size_t AFSK_MAX_STREAMS = 4096;                 // the bound of rr_channelizer_create
constexpr size_t AFSK_MAX_PUSH = (size_t)1 << 30;         // nstreams * n of one push

// What rr_afsk_demod_create refuses, said before any device is touched; nullptr: fine.
inline const char* afsk_check(size_t nstreams, size_t hilbert_ntaps, int window, float window_parm, float gain, const float* taps,
                              size_t ntaps, float offset) {
    if (nstreams < 1 || nstreams > AFSK_MAX_STREAMS) return "nstreams out of range";
    if (hilbert_ntaps < 2 || (hilbert_ntaps & 1) == 0) return "hilbert filter len must be odd and greater than 1";     // hilbert.rs:48
    if (hilbert_ntaps > (size_t)AFSK_MAX_HILBERT) return "hilbert filter len above 1023";
    if (window < 0 || window > 3 || !std::isfinite(window_parm)) return "unknown window, or a non-finite window parameter";
    if (!taps || ntaps < 1 || ntaps > (size_t)AFSK_MAX_TAPS) return "AfskDemod needs 1 to 4096 finite taps";
    for (size_t i = 0; i < ntaps; i++)
        if (!std::isfinite(taps[i])) return "AfskDemod needs 1 to 4096 finite taps";
    if (!std::isfinite(gain) || !std::isfinite(offset)) return "gain and offset must be finite";
    return nullptr;
}
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* afsk_check_push(size_t nstreams, const void* in, size_t in_stride, size_t n, const void* out, size_t out_stride) {
    if (n > AFSK_MAX_PUSH || nstreams * n > AFSK_MAX_PUSH) return "afsk demod: more than 2^30 samples in one push";
    if (in_stride < n) return "afsk demod: in_stride below n";
    if (out_stride < n) return "afsk demod: out_stride below n";
    if (n && (!in || !out)) return "afsk demod: null buffer";
    return nullptr;
}
// Elements from the first stream's first to the last stream's last: what a host push moves in one piece.  0 for n == 0.
inline size_t afsk_span(size_t nstreams, size_t stride, size_t n) { return n ? (nstreams - 1) * stride + n : 0; }
inline std::vector<float> afsk_reversed(const std::vector<float>& hil) { return std::vector<float>(hil.rbegin(), hil.rend()); }

// The handle on the host: the same carry pair, the same plan, every tile of the grid with every thread of its workgroup in turn.
struct AfskHost {
    size_t nstreams;
    AfskGeom g;
    std::vector<float> taps, hr, carry[2];
    int cur = 0;
    unsigned long long total = 0;                         // samples every stream has taken
    float gain, offset;
    // hil = hilbert_taps(make_window(..)), H entries
    AfskHost(size_t ns, const std::vector<float>& hil, float gn, const std::vector<float>& tp, float off)
        : nstreams(ns), g(afsk_geom((int)hil.size(), (int)tp.size())), taps(tp), hr(afsk_reversed(hil)), gain(gn), offset(off) {
        for (auto& c : carry) c.assign(ns * (size_t)g.C, 0.0f);
    }
    // -> produced (the same for every stream); a push that is refused changes nothing and throws its sentence
    size_t push(const float* in, size_t in_stride, size_t n, float* out, size_t out_stride) {
        if (const char* e = afsk_check_push(nstreams, in, in_stride, n, out, out_stride)) throw e;
        if (!n) return 0;
        AfskArgs a{};
        a.g = g;
        a.in = in; a.in_stride = (long)in_stride;
        a.out = out; a.out_stride = (long)out_stride;
        a.carry_in = carry[cur].data(); a.carry_out = carry[cur ^ 1].data();
        a.taps = taps.data(); a.hr = hr.data();
        a.gain = gain; a.offset = offset;
        afsk_plan(a, total, (long)n);
        const long ntiles = afsk_tiles(a.produced);
        std::vector<float> lds((size_t)g.lds_floats);
        for (long c = 0; c < (long)nstreams; c++)
            for (long tx = 0; tx < ntiles; tx++) {
                float* X = lds.data();
                float* D = X + g.x_floats;
                float* HR = D + g.d_floats;
                for (int t = 0; t < AFSK_NT; t++) afsk_load(a, c, tx, tx == ntiles - 1, t, X, D, HR);
                const int nk = afsk_tile_nk(a, tx), ng = afsk_tile_groups(a, nk);
                for (int t = 0; t < AFSK_NT; t++)
                    for (int gi = t; gi < ng; gi += AFSK_NT) afsk_demod(a, tx * AFSK_TILE, gi, X, HR, D);
                if (!nk) continue;
                for (int j = 0; j < g.L; j++) X[j] = taps[(size_t)j];
                for (int t = 0; t < AFSK_NT && AFSK_R * t < nk; t++) {
                    float y[AFSK_R];
                    afsk_lowpass(a, t, X, D, y);
                    for (int r = 0; r < AFSK_R && AFSK_R * t + r < nk; r++)
                        out[(size_t)c * out_stride + (size_t)(tx * AFSK_TILE + AFSK_R * t + r)] = y[r];
                }
            }
        cur ^= 1;
        total += n;
        return (size_t)a.produced;
    }
};

}  // namespace rr
