// frame_host.hpp — the host-only logic behind rr_hdlc_framer_bound, rr_hdlc_framer_push_dev and rr_hdlc_framer_records: the bound,
// the argument checks, the descriptors a push uploads, and what is done to the device's counters once they are in host memory.
// No HIP in here, so tests/cpp/test_frame_hostlogic.cpp builds it with the host sanitizers and drives it without a device.
// Every host buffer is sized from the packet count and the bound, which the host knows, never from a number the device wrote.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"

namespace rr {

constexpr size_t FRAME_MAX_BOUND = (size_t)1 << 30;       // elements of one push
constexpr int FRAME_ALL_FLAGS = RR_FRAME_FCS | RR_FRAME_G3RUH | RR_FRAME_NRZI | RR_FRAME_SYMBOLS;

// What rr_hdlc_framer_create refuses, said before any device is touched; nullptr: fine.
inline const char* frame_check_flags(int flags) { return flags & ~FRAME_ALL_FLAGS ? "unknown hdlc framer flags" : nullptr; }

// sum of 320 + 8 L + floor(8 L / 5), L = len + 2 with the FCS: reached by an all-ones payload.  Saturates at SIZE_MAX.
inline size_t frame_bound(int flags, const size_t* lens, size_t npackets) {
    const size_t fcs = flags & RR_FRAME_FCS ? 2 : 0, big = ~(size_t)0;
    size_t sum = 0;
    for (size_t p = 0; p < npackets; p++) {
        if (lens[p] > (big - 320) / 10 - fcs) return big;
        const size_t bits = 8 * (lens[p] + fcs), one = 320 + bits + bits / 5;
        if (one > big - sum) return big;
        sum += one;
    }
    return sum;
}

// What a push refuses (nothing may be launched then); nullptr: fine.  *bound: frame_bound of the batch.
inline const char* frame_check_push(int flags, size_t n_bytes, const size_t* starts, const size_t* lens, size_t npackets, size_t out_cap,
                                    size_t* bound) {
    *bound = 0;
    if (npackets && (!starts || !lens)) return "null packet descriptors";
    for (size_t p = 0; p < npackets; p++)
        if (starts[p] > n_bytes || lens[p] > n_bytes - starts[p]) return "packet outside the buffer";
    *bound = frame_bound(flags, lens, npackets);
    if (*bound > FRAME_MAX_BOUND) return "more than 2^30 framed bits in one push";
    if (out_cap < *bound) return "output shorter than the framed bits can be";
    return nullptr;
}

// The descriptors of a push, three arrays of 64-bit words back to back: starts[P], pb[P + 1] (the bytes of the packets in front,
// FCS bytes included), cpre[P + 1] (their CRC chunks of `chunk` payload bytes).
struct FramePlan {
    std::vector<unsigned long long> words;
    size_t P = 0, nbytes = 0, nchunks = 0;
    const unsigned long long* starts() const { return words.data(); }
    const unsigned long long* pb() const { return words.data() + P; }
    const unsigned long long* cpre() const { return words.data() + 2 * P + 1; }
};
inline void frame_plan(int flags, const size_t* starts, const size_t* lens, size_t npackets, size_t chunk, FramePlan& pl) {
    const size_t fcs = flags & RR_FRAME_FCS ? 2 : 0;
    pl.P = npackets;
    pl.words.assign(3 * npackets + 2, 0ull);
    unsigned long long* st = pl.words.data();
    unsigned long long* pb = st + npackets;
    unsigned long long* cp = pb + npackets + 1;
    size_t at = 0, ch = 0;
    for (size_t p = 0; p < npackets; p++) {
        st[p] = starts[p];
        pb[p] = at;
        cp[p] = ch;
        at += lens[p] + fcs;
        ch += (lens[p] + chunk - 1) / chunk;
    }
    pb[npackets] = at;
    cp[npackets] = ch;
    pl.nbytes = at;
    pl.nchunks = ch;
}

// The records of a push from what the device left: cb[b], b <= P, the stuffed bits in front of packet b (ascending), crc[p] the
// FCS, total the framed bits.  nullptr, or why the device's numbers cannot be trusted (then rec is empty).
inline const char* frame_records(int flags, const std::vector<size_t>& lens, const std::vector<unsigned>& cb,
                                 const std::vector<unsigned>& crc, unsigned long long total, size_t bound,
                                 std::vector<rr_frame_record>& rec, size_t* produced) {
    const size_t P = lens.size(), fcs = flags & RR_FRAME_FCS ? 2 : 0;
    rec.clear();
    *produced = 0;
    if (cb.size() != P + 1 || (fcs && crc.size() != P)) return "hdlc framer: counters of another push";
    size_t at = 0;
    std::vector<rr_frame_record> r(P);
    for (size_t p = 0; p < P; p++) {
        const size_t bits = 8 * (lens[p] + fcs);
        if (cb[p + 1] < cb[p] || cb[p + 1] - cb[p] > bits / 5) return "hdlc framer: stuffed bits beyond what the packet can hold";
        r[p].start = at;
        r[p].stuffed = cb[p + 1] - cb[p];
        r[p].len = 320 + bits + r[p].stuffed;
        r[p].fcs = fcs ? (unsigned short)(crc[p] & 0xffffu) : (unsigned short)0;
        at += r[p].len;
    }
    if (P && cb[0] != 0) return "hdlc framer: stuffed bits in front of the first packet";
    if (total != at || at > bound) return "hdlc framer: framed bits beyond the bound";
    rec.swap(r);
    *produced = at;
    return nullptr;
}
// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void frame_copy_out(const std::vector<rr_frame_record>& r, rr_frame_record* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_frame_record));
}

}  // namespace rr
