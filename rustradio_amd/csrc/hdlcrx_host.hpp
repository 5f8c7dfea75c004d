// hdlcrx_host.hpp — the host-only logic behind rr_hdlc_receiver_create / _push / _push_dev / _frames / _frame_bytes / _stats /
// _consumed: the refusals, the bounds of a push, the validation of everything the device wrote, and the clamped copy-outs.  No HIP
// in here, so tests/cpp/test_hdlcrx_hostlogic.cpp builds it with the host sanitizers and drives it without a device.  As in
// hdlc_host.hpp, every host buffer is sized from nstreams, n_cap, max_size and the carry bound the host tracks itself, never from a
// number the device wrote; what the device wrote is checked against those bounds BEFORE it is used as a size or an index.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"
#include "hdlc_host.hpp"

namespace rr {

constexpr size_t HDLCRX_MAX_STREAMS = 4096;
constexpr size_t HDLCRX_MAX_PUSH = (size_t)1 << 30;       // symbols of one push, all streams together
constexpr int HDLCRX_BIT_FLAGS = RR_BITS_INVERT | RR_BITS_NRZI | RR_BITS_DESCRAMBLE;
static_assert(sizeof(rr_hdlc_stream_frame) == 32, "rr_hdlc_stream_frame is 32 bytes");

// The refusals of the bit chain's parameters: bits_check (blocks_packet.cpp) says these for rr_bit_decoder_create as well.
inline const char* hdlcrx_check_bits(int flags, unsigned long long seed, unsigned len) {
    if (flags & ~HDLCRX_BIT_FLAGS) return "unknown bit decoder flags";
    if (flags & RR_BITS_DESCRAMBLE) {
        if (len >= 64) return "descrambler length out of range";                       // descrambler.rs:22 (assert)
        if (len < 63 && seed >> (len + 1)) return "seed wider than the register";
    }
    return nullptr;
}
// What rr_hdlc_receiver_create refuses, said before any device is touched; nullptr: fine.
inline const char* hdlcrx_check_create(size_t nstreams, int bit_flags, unsigned long long seed, unsigned len, size_t min_size,
                                       size_t max_size, int hdlc_flags) {
    if (nstreams == 0 || nstreams > HDLCRX_MAX_STREAMS) return "nstreams out of range";
    if (const char* e = hdlcrx_check_bits(bit_flags, seed, len)) return e;
    return hdlc_check_create(min_size, max_size, hdlc_flags);
}
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* hdlcrx_check_push(size_t nstreams, const void* syms, size_t stride, size_t n_cap) {
    if (stride < n_cap) return "hdlc receiver: stride shorter than n_cap";
    if (n_cap && nstreams > HDLCRX_MAX_PUSH / n_cap) return "hdlc receiver: more than 2^30 symbols in one push";
    if (n_cap && !syms) return "hdlc receiver: null symbols";
    return nullptr;
}

// The bounds of a push of at most n_cap symbols per stream behind at most `carry` carried bits (hdlc_next_carry over n_cap: one
// number serves all streams, a stream that got fewer symbols carries no more than one that got them all).
struct HdlcRxBounds {
    size_t nstreams = 0;
    HdlcBounds one;       // of one stream: hdlc_bounds(carry, n_cap)
    size_t frames = 0;    // of all streams
    size_t arena = 0;     // of all streams: stream c owns [c one.arena, (c + 1) one.arena)
};
inline HdlcRxBounds hdlcrx_bounds(size_t nstreams, size_t carry, size_t n_cap) {
    HdlcRxBounds b;
    b.nstreams = nstreams;
    b.one = hdlc_bounds(carry, n_cap);
    b.frames = nstreams * b.one.frames;
    b.arena = nstreams * b.one.arena;
    return b;
}
inline const char* hdlcrx_check_count(unsigned long long count, const HdlcRxBounds& b) {
    return count > b.frames ? "hdlc receiver: frame count beyond the bound" : nullptr;
}

// What the device says a stream has consumed so far against what it had consumed before the push: it moved on by at most n_cap.
// -> the symbols of this push (clamped to n_cap), or why not.
inline const char* hdlcrx_clamp_consumed(const unsigned long long* before, const unsigned long long* after, size_t nstreams, size_t n_cap,
                                         std::vector<size_t>& moved) {
    moved.assign(nstreams, 0);
    for (size_t c = 0; c < nstreams; c++) {
        if (after[c] < before[c]) { moved.assign(nstreams, 0); return "hdlc receiver: a stream position ran backwards"; }
        moved[c] = (size_t)std::min<unsigned long long>(after[c] - before[c], n_cap);
    }
    return nullptr;
}

// The records (in the device's order), the positions and the counters of a push: nullptr and rec sorted by (stream, pos), or why
// the device's numbers cannot be trusted (then rec is empty).  pos0[c]: stream c's position before the push, moved[c]: its symbols
// of this push (hdlcrx_clamp_consumed); before / after: 3 counters per stream.
inline const char* hdlcrx_validate(std::vector<rr_hdlc_stream_frame>& rec, const HdlcRxBounds& b, size_t max_size,
                                   const unsigned long long* pos0, const size_t* moved, const unsigned long long* before,
                                   const unsigned long long* after) {
    const char* bad = nullptr;
    if (rec.size() > b.frames) bad = "hdlc receiver: frame count beyond the bound";
    for (size_t i = 0; i < rec.size() && !bad; i++) {
        const rr_hdlc_stream_frame& r = rec[i];
        if (r.stream >= b.nstreams) { bad = "hdlc receiver: no such stream"; break; }
        const unsigned long long lo = (unsigned long long)r.stream * b.one.arena, hi = lo + b.one.arena;
        if (r.len > max_size) bad = "hdlc receiver: frame longer than max_size";
        else if (r.start < lo || r.start > hi || r.len > hi - r.start) bad = "hdlc receiver: frame outside its stream's arena";
        else if (r.pos < pos0[r.stream] || r.pos - pos0[r.stream] >= moved[r.stream]) bad = "hdlc receiver: frame position outside the push";
        else if (r.flags & ~1u) bad = "hdlc receiver: unknown record flags";
        else if (r.reserved) bad = "hdlc receiver: unknown record flags";
    }
    if (!bad) {
        std::sort(rec.begin(), rec.end(), [](const rr_hdlc_stream_frame& x, const rr_hdlc_stream_frame& y) {
            return x.stream != y.stream ? x.stream < y.stream : x.pos < y.pos;
        });
        for (size_t i = 1; i < rec.size() && !bad; i++)
            if (rec[i].stream == rec[i - 1].stream && rec[i].pos == rec[i - 1].pos) bad = "hdlc receiver: two frames at one position";
    }
    unsigned long long decoded = 0;
    for (size_t c = 0; c < b.nstreams && !bad; c++) {
        for (int k = 0; k < 3 && !bad; k++)
            if (after[3 * c + k] < before[3 * c + k]) bad = "hdlc receiver: a counter ran backwards";
        if (!bad) decoded += after[3 * c] - before[3 * c];
    }
    if (!bad && decoded != rec.size()) bad = "hdlc receiver: decoded counters and frame count disagree";
    if (bad) rec.clear();
    return bad;
}

// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void hdlcrx_copy_frames(const std::vector<rr_hdlc_stream_frame>& r, rr_hdlc_stream_frame* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_hdlc_stream_frame));
}
// one number per stream, the contract of rr_symbol_sync_produced
inline void hdlcrx_copy_u64(const std::vector<unsigned long long>& v, size_t column, size_t columns, unsigned long long* out, size_t cap,
                            size_t* total) {
    const size_t n = v.size() / columns;
    *total = n;
    for (size_t c = 0; c < n && c < cap && out; c++) out[c] = v[c * columns + column];
}

}  // namespace rr
