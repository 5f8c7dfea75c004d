// kiss_host.hpp — the host-only logic behind rr_kiss_decode_* and rr_kiss_encode_*: the argument checks, the sizes of a push, the
// descriptors an encode push uploads, and what is done to the device's numbers once they are in host memory.  No HIP in here, so
// tests/cpp/test_kiss_hostlogic.cpp builds it with the host sanitizers and drives it without a device.  Every host buffer is sized
// from the push's length, the carry bound and max_len, which the host knows, never from a number the device wrote.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"

namespace rr {

constexpr size_t KISS_MAX_PUSH = (size_t)1 << 30;         // bytes of one push; bytes of one encode bound
constexpr size_t KISS_MAX_MAX_LEN = (size_t)1 << 20;
constexpr size_t KISS_TILE = 4096;                        // (= KISS_T of kiss_core.hpp)

// ---- decode ----------------------------------------------------------------------------------------------------------------------------
// What rr_kiss_decode_create refuses, said before any device is touched; nullptr: fine.
inline const char* kiss_check_create(size_t max_len) {
    return max_len == 0 || max_len > KISS_MAX_MAX_LEN ? "kiss decode: max_len out of range (1 .. 2^20)" : nullptr;
}
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* kiss_check_push(const void* bytes, size_t n) {
    if (n > KISS_MAX_PUSH) return "kiss decode: more than 2^30 bytes in one push";
    if (n && !bytes) return "kiss decode: null input";
    return nullptr;
}
// The sizes of a push of n > 0 bytes behind at most `carry` carried ones.  A packet needs its closing FEND in the window and a port
// byte in front of it; its bytes are bytes of the virtual stream.
struct KissPlan {
    size_t nv_max, ntiles, rec_cap, arena_cap;
};
inline KissPlan kiss_plan(size_t carry, size_t n) {
    KissPlan p;
    p.nv_max = carry + n;
    p.ntiles = (p.nv_max + KISS_TILE - 1) / KISS_TILE;
    p.rec_cap = std::min(n, p.nv_max / 2);
    p.arena_cap = p.nv_max;
    return p;
}
// the carried bytes behind that push, at most
inline size_t kiss_next_carry(size_t carry, size_t n, size_t max_len) { return std::min(max_len, carry + n); }

// The device's two counts of a push (packets, arena bytes) against its plan; nullptr: they can size the read-back.
inline const char* kiss_check_count(const unsigned long long k[2], const KissPlan& p) {
    if (k[0] > p.rec_cap) return "kiss decode: more packets than the push can hold";
    if (k[1] > p.arena_cap) return "kiss decode: more packet bytes than the push can hold";
    return nullptr;
}
// The records of a push against everything the host knows: the window [at, at + n) of the stream, the carry bound, max_len, the
// counts, and the five counters before and behind it.  nullptr, or why the device's numbers cannot be trusted.
inline const char* kiss_validate(const std::vector<rr_kiss_packet>& r, const KissPlan& p, size_t max_len, unsigned long long at, size_t n,
                                 size_t carry, unsigned long long arena_bytes, const unsigned long long before[5],
                                 const unsigned long long now[5]) {
    if (r.size() > p.rec_cap || arena_bytes > p.arena_cap) return "kiss decode: counts beyond the push";
    unsigned long long sum = 0, prev_end = at;            // the first stream position a packet's gap may begin at, carry apart
    for (size_t i = 0; i < r.size(); i++) {
        const rr_kiss_packet& k = r[i];
        if (k.pos < at || k.pos - at >= n) return "kiss decode: packet outside the push";
        if (k.in_bytes >= max_len || k.len > k.in_bytes || k.in_bytes - k.len > k.in_bytes / 2) return "kiss decode: packet lengths out of range";
        // the gap (port byte, then in_bytes) ends at pos and begins behind the previous packet's FEND, or inside the carry
        const unsigned long long room = k.pos < prev_end ? 0 : k.pos - prev_end + (i == 0 ? carry : 0);
        if ((unsigned long long)k.in_bytes + 1 > room) return "kiss decode: packets overlap or run backwards";
        if (k.start != sum) return "kiss decode: arena not packed in stream order";
        if (k.port > 15 || k.reserved != 0) return "kiss decode: port out of range";
        sum += k.len;
        prev_end = k.pos + 1;
    }
    if (sum != arena_bytes) return "kiss decode: arena bytes disagree with the records";
    for (int q = 0; q < 5; q++)
        if (now[q] < before[q]) return "kiss decode: a counter ran backwards";
    const unsigned long long d[5] = {now[0] - before[0], now[1] - before[1], now[2] - before[2], now[3] - before[3], now[4] - before[4]};
    if (d[1] != r.size() || d[0] != d[1] + d[2] + d[3] || d[0] > n || d[4] > n) return "kiss decode: counters disagree with the records";
    return nullptr;
}
// The contract of rr_wpcr_results: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
template <class T> inline void kiss_copy_out(const std::vector<T>& r, T* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(T));
}

// ---- encode ----------------------------------------------------------------------------------------------------------------------------
// sum of 3 + 2 L: reached by a payload of FEND / FESC bytes only.  Saturates at SIZE_MAX.
inline size_t kiss_encode_bound(const size_t* lens, size_t npackets) {
    const size_t big = ~(size_t)0;
    size_t sum = 0;
    for (size_t p = 0; p < npackets; p++) {
        if (lens[p] > (big - 3) / 2) return big;
        const size_t one = 3 + 2 * lens[p];
        if (one > big - sum) return big;
        sum += one;
    }
    return sum;
}
// What a push refuses (nothing may be launched then); nullptr: fine.  *bound: kiss_encode_bound of the batch.
inline const char* kiss_encode_check_push(size_t n_bytes, const size_t* starts, const size_t* lens, size_t npackets, size_t out_cap,
                                          size_t* bound) {
    *bound = 0;
    if (npackets && (!starts || !lens)) return "kiss encode: null packet descriptors";
    if (n_bytes > KISS_MAX_PUSH) return "kiss encode: more than 2^30 bytes in one push";
    for (size_t p = 0; p < npackets; p++)
        if (starts[p] > n_bytes || lens[p] > n_bytes - starts[p]) return "kiss encode: packet outside the buffer";
    *bound = kiss_encode_bound(lens, npackets);
    if (*bound > KISS_MAX_PUSH) return "kiss encode: more than 2^30 encoded bytes in one push";
    if (out_cap < *bound) return "kiss encode: output shorter than the encoded bytes can be";
    return nullptr;
}
// The descriptors of a push, three arrays of 64-bit words back to back: starts[P], pb[P + 1] (the bytes of the packets in front),
// ports[P] (0 without `ports`).
struct KissEncPlan {
    std::vector<unsigned long long> words;
    size_t P = 0, nbytes = 0;
};
inline void kiss_encode_plan(const size_t* starts, const size_t* lens, const unsigned* ports, size_t npackets, KissEncPlan& pl) {
    pl.P = npackets;
    pl.words.assign(3 * npackets + 1, 0ull);
    unsigned long long* st = pl.words.data();
    unsigned long long* pb = st + npackets;
    unsigned long long* po = pb + npackets + 1;
    size_t at = 0;
    for (size_t p = 0; p < npackets; p++) {
        st[p] = starts[p];
        pb[p] = at;
        po[p] = ports ? ports[p] : 0u;
        at += lens[p];
    }
    pb[npackets] = at;
    pl.nbytes = at;
}
// The records of a push from what the device left: cb[b], b <= P, the escaped bytes in front of packet b (ascending), total the
// encoded bytes.  nullptr, or why the device's numbers cannot be trusted (then rec is empty).
inline const char* kiss_encode_records(const std::vector<size_t>& lens, const std::vector<unsigned>& ports, const std::vector<unsigned>& cb,
                                       unsigned long long total, size_t bound, std::vector<rr_kiss_frame_record>& rec, size_t* produced) {
    const size_t P = lens.size();
    rec.clear();
    *produced = 0;
    if (cb.size() != P + 1 || ports.size() != P) return "kiss encode: counters of another push";
    if (P && cb[0] != 0) return "kiss encode: escaped bytes in front of the first packet";
    size_t at = 0;
    std::vector<rr_kiss_frame_record> r(P);
    for (size_t p = 0; p < P; p++) {
        if (cb[p + 1] < cb[p] || cb[p + 1] - cb[p] > lens[p]) return "kiss encode: escaped bytes beyond what the packet can hold";
        r[p].start = at;
        r[p].escaped = cb[p + 1] - cb[p];
        r[p].len = 3 + lens[p] + r[p].escaped;
        r[p].port = ports[p] < 16 ? ports[p] : 0u;
        at += r[p].len;
    }
    if (total != at || at > bound) return "kiss encode: encoded bytes beyond the bound";
    rec.swap(r);
    *produced = at;
    return nullptr;
}

}  // namespace rr
