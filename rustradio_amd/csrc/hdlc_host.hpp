// hdlc_host.hpp — the host-only logic behind rr_hdlc_deframer_create / _push / _push_dev, rr_hdlc_frames, rr_hdlc_frame_bytes and
// rr_hdlc_stats: the refusals, the carry bound, the bounds and the workspace plan of a push (which rr_hdlc_receiver sizes its
// streams' shares by as well), the validation of everything the device wrote, and the clamped copy-outs.  No HIP in here, so
// tests/cpp/test_hdlc_hostlogic.cpp builds it with the host sanitizers and drives it without a device.  Every host buffer is sized from the push length, max_size and the carry length the host tracks itself, never from a
// number the device wrote; what the device wrote is checked against those bounds BEFORE it is used as a size or an index.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"
#include "hdlc_core.hpp"
#include "hdlc_dims.hpp"

namespace rr {

constexpr size_t HDLC_MAX_PUSH = (size_t)1 << 30;         // bits of one push
constexpr size_t HDLC_MAX_SIZE = 65535;
constexpr int HDLC_ALL_FLAGS = RR_HDLC_KEEP_CHECKSUM | RR_HDLC_FIX_BITS;
static_assert(sizeof(rr_hdlc_frame) == 24, "rr_hdlc_frame is 24 bytes");

// What rr_hdlc_deframer_create refuses, said before any device is touched; nullptr: fine.  (min_size and max_size 0 are legal:
// HdlcDeframer::new takes any usize.)
inline const char* hdlc_check_create(size_t /*min_size*/, size_t max_size, int flags) {
    if (flags & ~HDLC_ALL_FLAGS) return "unknown hdlc deframer flags";
    if (max_size > HDLC_MAX_SIZE) return "hdlc deframer: max_size beyond 65535";
    return nullptr;
}
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* hdlc_check_push(const void* bits, size_t n) {
    if (n > HDLC_MAX_PUSH) return "hdlc deframer: more than 2^30 bits in one push";
    if (n && !bits) return "hdlc deframer: null bits";
    return nullptr;
}

// The most bits a handle carries from push to push: HDLC_HALO bits in front of the open gap, then at most hdlc_reach raw bits of
// it — a longer gap has reset whatever it holds and is cut down to the halo (hdlc_carry_plan).  With M = 8 max_size + 1 this
// is M + floor((M - 1) / 5) + 16; the stuffed all-ones frame gets there.
inline size_t hdlc_carry_bits(size_t max_size) { return (size_t)HDLC_HALO + (size_t)hdlc_reach(max_size); }
static_assert(HDLC_HALO == 8, "carry_bits = reset bits + 16");

// The bounds of a push of n bits behind at most `carry` carried ones (a host-side count: hdlc_next_carry).
struct HdlcBounds {
    size_t nv = 0;        // virtual bits
    size_t frames = 0;    // emitting flag ends lie in the push's own bits, at least 8 apart
    size_t arena = 0;     // a frame lies at byte floor((s + 1) / 8) and ends in front of byte floor((f - 7) / 8) + 1 <= nv / 8
};
inline HdlcBounds hdlc_bounds(size_t carry, size_t n) {
    HdlcBounds b;
    b.nv = carry + n;
    b.frames = (n + 7) / 8;
    b.arena = b.nv / 8;
    return b;
}
inline size_t hdlc_next_carry(size_t carry, size_t n, size_t max_size) { return std::min(hdlc_carry_bits(max_size), carry + n); }

// The workspace of ONE stream's share of such a push, in the units the kernels index by (HdlcArgs, kernels.hpp): every buffer a
// handle reserves and every pitch and capacity it hands to the device is one of these numbers, times its streams.
struct HdlcPlan {
    HdlcBounds one;       // hdlc_bounds(carry, n): nv_max, rec_cap and arena_cap
    size_t ntiles = 0;    // tiles of HDLC_T virtual bits: tilecnt / offs
    size_t nwords = 0;    // words of raw / fl / ab / sf: 64 per tile, and one behind the last tile's
    size_t ecap = 0;      // flag ends at least 7 bits apart, two to spare: ends / gmap / pmap, and ends_cap
    size_t nblocks = 0;   // blocks of HDLC_GB gaps: bmap / bstate
    size_t carry_cap = 0; // bytes of cin / cout
};
inline HdlcPlan hdlc_plan(size_t carry, size_t n, size_t max_size) {
    HdlcPlan p;
    p.one = hdlc_bounds(carry, n);
    p.ntiles = (p.one.nv + HDLC_T - 1) / HDLC_T;
    p.nwords = p.ntiles * (HDLC_T / 64) + 1;
    p.ecap = p.one.nv / 7 + 2;
    p.nblocks = (p.ecap + HDLC_GB - 1) / HDLC_GB;
    p.carry_cap = hdlc_carry_bits(max_size);
    return p;
}

// The frame count the device left, before it sizes anything.
inline const char* hdlc_check_count(unsigned long long count, const HdlcBounds& b) {
    return count > b.frames ? "hdlc deframer: frame count beyond the bound" : nullptr;
}
// The records (in the device's order) and the counters of a push of n bits at stream position w0: nullptr and rec sorted by pos,
// or why the device's numbers cannot be trusted (then rec is empty).  A delivered frame has at most max_size - 1 bytes with or
// without RR_HDLC_KEEP_CHECKSUM (one of exactly max_size has reset the machine first), so max_size bounds len in both cases.
inline const char* hdlc_validate(std::vector<rr_hdlc_frame>& rec, const HdlcBounds& b, size_t max_size, unsigned long long w0, size_t n,
                                 const unsigned long long before[3], const unsigned long long after[3]) {
    const char* bad = nullptr;
    if (rec.size() > b.frames) bad = "hdlc deframer: frame count beyond the bound";
    for (size_t i = 0; i < rec.size() && !bad; i++) {
        const rr_hdlc_frame& r = rec[i];
        if (r.len > max_size) bad = "hdlc deframer: frame longer than max_size";
        else if (r.start > b.arena || r.len > b.arena - r.start) bad = "hdlc deframer: frame outside the arena";
        else if (r.pos < w0 || r.pos - w0 >= n) bad = "hdlc deframer: frame position outside the push";
        else if (r.flags & ~1u) bad = "hdlc deframer: unknown record flags";
    }
    if (!bad) {
        std::sort(rec.begin(), rec.end(), [](const rr_hdlc_frame& x, const rr_hdlc_frame& y) { return x.pos < y.pos; });
        for (size_t i = 1; i < rec.size() && !bad; i++)
            if (rec[i].pos == rec[i - 1].pos) bad = "hdlc deframer: two frames at one position";
    }
    for (int k = 0; k < 3 && !bad; k++)
        if (after[k] < before[k]) bad = "hdlc deframer: a counter ran backwards";
    if (!bad && after[0] - before[0] != rec.size()) bad = "hdlc deframer: decoded counter and frame count disagree";
    if (bad) rec.clear();
    return bad;
}

// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void hdlc_copy_frames(const std::vector<rr_hdlc_frame>& r, rr_hdlc_frame* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_hdlc_frame));
}
inline void hdlc_copy_bytes(const std::vector<unsigned char>& a, unsigned char* out, size_t cap, size_t* total) {
    *total = a.size();
    const size_t k = std::min(cap, a.size());
    if (k && out) std::memcpy(out, a.data(), k);
}

}  // namespace rr
