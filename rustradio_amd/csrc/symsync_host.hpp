// symsync_host.hpp — the host-only logic behind rr_symbol_sync_create / _push / _push_dev / _produced: the refusals, the stride
// arithmetic and the clamped copy-out of the counts.  No HIP in here, so tests/cpp/test_symsync_hostlogic.cpp builds it with the
// host sanitizers and drives it without a device.  Every size the host uses comes from the caller's n, strides and nstreams; a
// count the device wrote is clamped to n before anybody uses it as a length.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "symsync_core.hpp"

namespace rr {

constexpr size_t SYNC_MAX_STREAMS = 4096;                 // the bound of rr_channelizer_create
constexpr size_t SYNC_MAX_PUSH = (size_t)1 << 31;         // samples of one stream in one push: below this (window indices are u32)

// What rr_symbol_sync_create refuses, said before any device is touched; nullptr: fine.
inline const char* symsync_check(float sps, float max_deviation, const float* taps, size_t ntaps, size_t nstreams) {
    if (!(sps > 1.0f)) return "sps must be above 1";                                         // symbol_sync.rs:78 (NaN fails it too)
    // (a deviation: the reference takes anything and loops forever once clock <= 0.  With mi >= sps / 2 > 0.5 every `while` of
    //  work() terminates in f32.)
    if (!(max_deviation >= 0.0f && max_deviation <= sps * 0.5f)) return "max_deviation out of range";
    if (!taps || ntaps < 1 || ntaps > (size_t)SYNC_MAX_TAPS) return "SymbolSync needs 1 to 8 finite taps";
    for (size_t i = 0; i < ntaps; i++)
        if (!std::isfinite(taps[i])) return "SymbolSync needs 1 to 8 finite taps";
    if (nstreams < 1 || nstreams > SYNC_MAX_STREAMS) return "nstreams out of range";
    return nullptr;
}
inline SyncParams symsync_params(float sps, float max_deviation, const float* taps, size_t ntaps) {
    SyncParams p{};
    p.sps = sps;
    p.max_dev = max_deviation;
    p.ntaps = (int)ntaps;
    for (size_t i = 0; i < ntaps; i++) p.taps[i] = taps[i];
    sync_derive(p);
    return p;
}

// What a push refuses (nothing may be launched then); nullptr: fine.  A sample emits at most one symbol, so out_stride >= n
// is room for everything.
inline const char* symsync_check_push(const void* in, size_t in_stride, size_t n, const void* syms, size_t out_stride) {
    if (n >= SYNC_MAX_PUSH) return "symbol sync: 2^31 samples or more in one push";
    if (in_stride < n) return "symbol sync: in_stride below n";
    if (out_stride < n) return "symbol sync: out_stride below n";
    if (n && (!in || !syms)) return "symbol sync: null buffer";
    return nullptr;
}
// Elements from the first stream's first to the last stream's last: what a host push moves in one piece.  0 for n == 0.
inline size_t symsync_span(size_t nstreams, size_t stride, size_t n) { return n ? (nstreams - 1) * stride + n : 0; }
// Words of one stream's signs.
inline size_t symsync_words(size_t n) { return (n + 63) / 64; }

// The counts the device left, clamped to the push's n, into `clean`.
inline void symsync_clamp_counts(const unsigned long long* raw, size_t nstreams, size_t n, std::vector<size_t>& clean) {
    clean.resize(nstreams);
    for (size_t c = 0; c < nstreams; c++) clean[c] = (size_t)std::min<unsigned long long>(raw[c], n);
}
// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void symsync_copy_counts(const std::vector<size_t>& counts, size_t* out, size_t cap, size_t* total) {
    *total = counts.size();
    const size_t k = std::min(cap, counts.size());
    for (size_t c = 0; c < k && out; c++) out[c] = counts[c];
}

}  // namespace rr
