// il2p_host.hpp — the host-only logic behind rr_il2p_receiver_create / _push / _push_dev / _headers / _stats / _consumed: the
// refusals, the bounds of a push, the validation of everything the device wrote, the ordering and the clamped copy-outs.  No HIP in
// here, so tests/cpp/test_il2p_hostlogic.cpp builds it with the host sanitizers and drives it without a device.  Every host buffer
// is sized from nstreams and n_cap, never from a number the device wrote; what the device wrote is checked against those bounds
// BEFORE it is used as a size or an index.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"
#include "il2p_core.hpp"

namespace rr {

constexpr size_t IL2P_MAX_STREAMS = 4096;
constexpr size_t IL2P_MAX_PUSH = (size_t)1 << 30;         // symbols of one push, all streams together
static_assert(sizeof(rr_il2p_header) == 64 && sizeof(Il2pRec) == sizeof(rr_il2p_header), "rr_il2p_header is 64 bytes");
static_assert(offsetof(Il2pRec, pos) == offsetof(rr_il2p_header, pos) && offsetof(Il2pRec, stream) == offsetof(rr_il2p_header, stream) &&
              offsetof(Il2pRec, payload_size) == offsetof(rr_il2p_header, payload_size) && offsetof(Il2pRec, pid) == offsetof(rr_il2p_header, pid) &&
              offsetof(Il2pRec, control) == offsetof(rr_il2p_header, control) && offsetof(Il2pRec, flags) == offsetof(rr_il2p_header, flags) &&
              offsetof(Il2pRec, diffs) == offsetof(rr_il2p_header, diffs) && offsetof(Il2pRec, dst_ssid) == offsetof(rr_il2p_header, dst_ssid) &&
              offsetof(Il2pRec, src_ssid) == offsetof(rr_il2p_header, src_ssid) && offsetof(Il2pRec, raw) == offsetof(rr_il2p_header, raw) &&
              offsetof(Il2pRec, dst) == offsetof(rr_il2p_header, dst) && offsetof(Il2pRec, src) == offsetof(rr_il2p_header, src) &&
              offsetof(Il2pRec, reserved) == offsetof(rr_il2p_header, reserved),
              "Il2pRec is rr_il2p_header");

// What rr_il2p_receiver_create refuses, said before any device is touched; nullptr: fine.  allowed_diffs takes any value.
inline const char* il2p_check_create(size_t nstreams, int bit_flags) {
    if (nstreams == 0 || nstreams > IL2P_MAX_STREAMS) return "nstreams out of range";
    if (bit_flags & ~RR_BITS_INVERT) return "il2p receiver: unknown bit flags";
    return nullptr;
}
// 24 and above: every position from 23 on matches
inline unsigned il2p_clamp_allowed(size_t allowed_diffs) { return (unsigned)std::min<size_t>(allowed_diffs, IL2P_SYNC_BITS); }
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* il2p_check_push(size_t nstreams, const void* syms, size_t stride, size_t n_cap) {
    if (stride < n_cap) return "il2p receiver: stride shorter than n_cap";
    if (n_cap && nstreams > IL2P_MAX_PUSH / n_cap) return "il2p receiver: more than 2^30 symbols in one push";
    if (n_cap && !syms) return "il2p receiver: null symbols";
    return nullptr;
}

// The bounds of a push of at most n_cap symbols per stream.
struct Il2pBounds {
    size_t nstreams = 0, n_cap = 0;
    size_t tiles = 0;         // of one stream
    size_t words = 0;         // of one stream's virtual stream: the carry, the tiles, one word a header's window may touch
    size_t per_stream = 0;    // headers of one stream, at most
    size_t headers = 0;       // of all streams
};
// A header ends inside the push when its tag lies in [-120, n - 121] relative to the push, and two tags are 121 apart at least:
// floor((n + 119) / 121) + 1 covers it with one to spare.
inline size_t il2p_max_headers(size_t n) { return n ? (n + 119) / 121 + 1 : 0; }
inline Il2pBounds il2p_bounds(size_t nstreams, size_t n_cap) {
    Il2pBounds b;
    b.nstreams = nstreams;
    b.n_cap = n_cap;
    b.tiles = (n_cap + IL2P_T - 1) / IL2P_T;
    b.words = IL2P_CARRY_WORDS + b.tiles * IL2P_TW + 1;
    b.per_stream = il2p_max_headers(n_cap);
    b.headers = nstreams * b.per_stream;
    return b;
}
inline const char* il2p_check_count(unsigned long long count, const Il2pBounds& b) {
    return count > b.headers ? "il2p receiver: header count beyond the bound" : nullptr;
}

// What the device says a stream has consumed so far against what it had consumed before the push: it moved on by at most n_cap.
inline const char* il2p_clamp_consumed(const unsigned long long* before, const unsigned long long* after, size_t nstreams, size_t n_cap,
                                       std::vector<size_t>& moved) {
    moved.assign(nstreams, 0);
    for (size_t c = 0; c < nstreams; c++) {
        if (after[c] < before[c]) { moved.assign(nstreams, 0); return "il2p receiver: a stream position ran backwards"; }
        moved[c] = (size_t)std::min<unsigned long long>(after[c] - before[c], n_cap);
    }
    return nullptr;
}

// The records (in the device's order) of a push: nullptr and rec sorted by (stream, pos), or why the device's numbers cannot be
// trusted (then rec is empty).  pos0[c]: stream c's position before the push, moved[c]: its symbols of this push.  A header
// belongs to the push when its 120th bit, at pos + 120, lies inside it.
inline const char* il2p_validate(std::vector<rr_il2p_header>& rec, const Il2pBounds& b, const unsigned long long* pos0, const size_t* moved) {
    const char* bad = nullptr;
    if (rec.size() > b.headers) bad = "il2p receiver: header count beyond the bound";
    for (size_t i = 0; i < rec.size() && !bad; i++) {
        const rr_il2p_header& r = rec[i];
        if (r.stream >= b.nstreams) { bad = "il2p receiver: no such stream"; break; }
        const unsigned long long end = r.pos + IL2P_HEADER_BITS;
        if (r.pos < IL2P_SYNC_BITS - 1 || end < r.pos) bad = "il2p receiver: header position outside the stream";
        else if (end < pos0[r.stream] || end - pos0[r.stream] >= moved[r.stream]) bad = "il2p receiver: header position outside the push";
        else if (r.diffs > IL2P_SYNC_BITS || r.payload_size > 1023 || r.pid > 15 || r.control > 127 || (r.flags & ~7u) || r.dst_ssid > 15 || r.src_ssid > 15)
            bad = "il2p receiver: header field out of range";
    }
    if (!bad) {
        std::sort(rec.begin(), rec.end(), [](const rr_il2p_header& x, const rr_il2p_header& y) {
            return x.stream != y.stream ? x.stream < y.stream : x.pos < y.pos;
        });
        for (size_t i = 1; i < rec.size() && !bad; i++)
            if (rec[i].stream == rec[i - 1].stream && rec[i].pos - rec[i - 1].pos < (unsigned long long)IL2P_STATES)
                bad = "il2p receiver: two headers closer than 121";
    }
    if (bad) rec.clear();
    return bad;
}

// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void il2p_copy_headers(const std::vector<rr_il2p_header>& r, rr_il2p_header* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_il2p_header));
}
// one number per stream, the contract of rr_symbol_sync_produced
inline void il2p_copy_u64(const std::vector<unsigned long long>& v, size_t column, size_t columns, unsigned long long* out, size_t cap,
                          size_t* total) {
    const size_t n = v.size() / columns;
    *total = n;
    for (size_t c = 0; c < n && c < cap && out; c++) out[c] = v[c * columns + column];
}

}  // namespace rr
