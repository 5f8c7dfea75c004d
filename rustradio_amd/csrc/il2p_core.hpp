// il2p_core.hpp — the arithmetic of rr_il2p_receiver: plain functions, no HIP types, shared by kernels_il2p.hip and
// tests/cpp/emu_il2p.cpp, which holds them under g++ to bit-serial code: CorrelateAccessCodeTag (src/correlate_access_code.rs:93-118)
// on il2p_deframer::SYNC_WORD (src/il2p_deframer.rs:16-18) and Il2pDeframer (src/il2p_deframer.rs:101-128, 172-237, 247-319).
//   il2p_match_exact / il2p_diffs_at / il2p_match_word    where the sync word ends, 64 positions at once
//   il2p_tile_map / il2p_map_then                         the chain rule of one tile as a map over 121 entry states, and its composition
//   il2p_next_tag                                          the walk both the map and the emit stage take
//   il2p_descramble / il2p_header_bytes / il2p_parse       120 line bits -> 15 bytes -> the record
// A stream's symbols of a push stand behind the IL2P_CARRY bits the stream so far left (zeros before its start): the VIRTUAL
// stream.  Bit v of it is bit v & 63 of word v >> 6; symbol i of the push is v = IL2P_CARRY + i.
#pragma once
#if defined(__HIPCC__)
#define RR_IL2P_HD __host__ __device__ inline
#else
#define RR_IL2P_HD inline
#endif

namespace rr {

typedef unsigned long long il2p_u64;

constexpr int IL2P_SYNC_BITS = 24;                    // il2p_deframer.rs:16-18
constexpr unsigned IL2P_SYNC = 0xF15E48u;             // ... oldest bit first
constexpr int IL2P_HEADER_BITS = 120;                 // il2p_deframer.rs:10
constexpr int IL2P_STATES = IL2P_HEADER_BITS + 1;     // positions at a tile's start that are still blocked: 0 .. 120
constexpr int IL2P_CARRY_WORDS = 3;
constexpr int IL2P_CARRY = 64 * IL2P_CARRY_WORDS;     // >= 143: 23 bits for the correlator, 120 for an open header's tag and bits
constexpr int IL2P_TW = 64;                           // words of a tile
constexpr int IL2P_T = 64 * IL2P_TW;                  // symbols of a tile (rr_il2p_receiver_dims)
constexpr int IL2P_MAP_PITCH = 128;                   // bytes of one tile's map (121 used)

// a stream's state between pushes: IL2P_ST_N words per stream
enum { IL2P_ST_POS = 0,                               // symbols of the stream so far
       IL2P_ST_SEEN = 1,                              // min(pos, 24): correlate_access_code.rs' slide.len()
       IL2P_ST_BLOCKED = 2,                           // max(free_from - pos, 0) in 0 .. 120; > 0: a header is open, its tag at
                                                      // pos + blocked - 121
       IL2P_ST_BITS = 3,                              // IL2P_CARRY_WORDS words: the last IL2P_CARRY sliced bits, newest last
       IL2P_ST_N = 8 };

// The record of one header: rr_il2p_header (include/rustradio_amd.h).
struct Il2pRec {
    unsigned long long pos;
    unsigned stream;
    unsigned short payload_size;
    unsigned char pid, control, flags, diffs, dst_ssid, src_ssid;
    unsigned char raw[15];
    char dst[7], src[7];
    unsigned char reserved[15];
};
static_assert(sizeof(Il2pRec) == 64, "Il2pRec is rr_il2p_header");

RR_IL2P_HD int il2p_popc(il2p_u64 x) { return __builtin_popcountll(x); }
RR_IL2P_HD int il2p_ctz(il2p_u64 x) { return __builtin_ctzll(x); }

// the bits of the word at virtual position vb that lie in front of virtual position k
RR_IL2P_HD il2p_u64 il2p_below(long vb, long k) {
    const long d = k - vb;
    return d <= 0 ? 0ull : d >= 64 ? ~0ull : (1ull << d) - 1ull;
}
// the 64 bits of W that start at bit position a: bit 0 of the result is bit a (W[(a >> 6) + 1] must be readable)
RR_IL2P_HD il2p_u64 il2p_win(const il2p_u64* W, long a) {
    const long wi = a >> 6, off = a & 63;
    return off ? (W[wi] >> off) | (W[wi + 1] << (64 - off)) : W[wi];
}

// ---- the correlator ---------------------------------------------------------------------------------------------------------------
// SYNC_WORD[k] stands at position i - 23 + k of a window that ends at i.  The word whose bit j is b[i - d] for i = 64 w + j:
RR_IL2P_HD il2p_u64 il2p_back(il2p_u64 cur, il2p_u64 prev, int d) { return d ? (cur << d) | (prev >> (64 - d)) : cur; }
// allowed_diffs == 0: 24 shifted XNOR terms ANDed.  prev: the word in front of cur.
RR_IL2P_HD il2p_u64 il2p_match_exact(il2p_u64 cur, il2p_u64 prev) {
    il2p_u64 m = ~0ull;
    for (int k = 0; k < IL2P_SYNC_BITS; k++) {
        const il2p_u64 sh = il2p_back(cur, prev, IL2P_SYNC_BITS - 1 - k);
        m &= (IL2P_SYNC >> (IL2P_SYNC_BITS - 1 - k) & 1u) ? sh : ~sh;
    }
    return m;
}
// diffs of the window that ends at bit j of cur (correlate_access_code.rs:104-109)
RR_IL2P_HD int il2p_diffs_at(il2p_u64 cur, il2p_u64 prev, int j) {
    // the 24 bits ending at j, newest in bit 0 ... oldest in bit 23, which is how IL2P_SYNC reads with its oldest bit first
    unsigned w = 0;
    for (int d = 0; d < IL2P_SYNC_BITS; d++) {
        const int p = j - d;
        const unsigned bit = (unsigned)((p >= 0 ? cur >> p : prev >> (64 + p)) & 1ull);
        w |= bit << d;
    }
    return __builtin_popcount(w ^ IL2P_SYNC);
}
// The match word of the 64 positions whose virtual positions start at vb: bit j set when position vb + j carries a tag.  first:
// the first virtual position at which 24 bits of the stream have been seen; nv: the end of the virtual stream.
RR_IL2P_HD il2p_u64 il2p_match_word(il2p_u64 cur, il2p_u64 prev, unsigned allowed, long vb, long first, long nv) {
    il2p_u64 m = 0;
    if (allowed >= (unsigned)IL2P_SYNC_BITS) m = ~0ull;
    else if (allowed == 0) m = il2p_match_exact(cur, prev);
    else
        for (int j = 0; j < 64; j++)
            if ((unsigned)il2p_diffs_at(cur, prev, j) <= allowed) m |= 1ull << j;
    return m & ~il2p_below(vb, first) & il2p_below(vb, nv);
}
// where 24 bits have been seen: symbol i of the push is the (seen0 + i + 1)-th bit
RR_IL2P_HD long il2p_first_valid(il2p_u64 seen0) { return (long)IL2P_CARRY + (seen0 >= 24 ? 0 : 23 - (long)seen0); }

// ---- the chain rule ---------------------------------------------------------------------------------------------------------------
// The first tag at or behind position p of a tile of len positions whose match words are m (bit q of word q >> 6): its position,
// or len when there is none.
RR_IL2P_HD long il2p_next_tag(const il2p_u64* m, long len, long p) {
    if (p >= len) return len;
    long w = p >> 6;
    il2p_u64 x = m[w] & ~il2p_below(0, p & 63);
    const long nw = (len + 63) >> 6;
    while (!x) {
        if (++w >= nw) return len;
        x = m[w];
    }
    const long q = (w << 6) + il2p_ctz(x);
    return q < len ? q : len;
}
// The tile entered with its first e positions blocked (free_from = tile start + e): the positions blocked at the start of the
// next tile.  Every accepted tag at q blocks up to q + 120 (il2p_deframer.rs:194, 199-204).
RR_IL2P_HD int il2p_tile_exit(const il2p_u64* m, long len, int e) {
    long p = e;
    for (;;) {
        if (p >= len) return (int)(p - len);
        const long q = il2p_next_tag(m, len, p);
        if (q >= len) return 0;
        p = q + IL2P_STATES;
    }
}
RR_IL2P_HD void il2p_tile_map(const il2p_u64* m, long len, unsigned char* map) {
    for (int e = 0; e < IL2P_STATES; e++) map[e] = (unsigned char)il2p_tile_exit(m, len, e);
}
// out = a, then b
RR_IL2P_HD void il2p_map_then(const unsigned char* a, const unsigned char* b, unsigned char* out) {
    for (int e = 0; e < IL2P_STATES; e++) out[e] = b[a[e]];
}

// ---- the header -------------------------------------------------------------------------------------------------------------------
// Lfsr::new(0x108, 0x1f0) (il2p_deframer.rs:107-128, 257) in closed form: out[k] = in[k] ^ in[k - 4] ^ in[k - 9] ^ c[k], c = 1 for
// k = 4 .. 8 (the seed leaving the register).  x0: header bits 0 .. 63 (bit k in bit k), x1: bits 64 .. 119.
RR_IL2P_HD void il2p_descramble(il2p_u64 x0, il2p_u64 x1, il2p_u64* y0, il2p_u64* y1) {
    x1 &= (1ull << 56) - 1ull;
    *y0 = x0 ^ (x0 << 4) ^ (x0 << 9) ^ 0x1f0ull;
    *y1 = (x1 ^ (x1 << 4 | x0 >> 60) ^ (x1 << 9 | x0 >> 55)) & ((1ull << 56) - 1ull);
}
RR_IL2P_HD unsigned char il2p_rev8(unsigned b) {
    b = (b & 0xf0u) >> 4 | (b & 0x0fu) << 4;
    b = (b & 0xccu) >> 2 | (b & 0x33u) << 2;
    b = (b & 0xaau) >> 1 | (b & 0x55u) << 1;
    return (unsigned char)b;
}
// bits_to_bytes (il2p_deframer.rs:130-141): MSB first
RR_IL2P_HD void il2p_header_bytes(il2p_u64 y0, il2p_u64 y1, unsigned char* raw /* 15 */) {
    for (int j = 0; j < 8; j++) raw[j] = il2p_rev8((unsigned)(y0 >> (8 * j)) & 0xffu);
    for (int j = 0; j < 7; j++) raw[8 + j] = il2p_rev8((unsigned)(y1 >> (8 * j)) & 0xffu);
}
// decode_callsign (il2p_deframer.rs:265-274): every 6-bit zero is dropped; NUL padded
RR_IL2P_HD void il2p_callsign(const unsigned char* d, char* out /* 7 */) {
    int n = 0;
    for (int i = 0; i < 6; i++) {
        const unsigned ch = d[i] & 63u;
        if (ch) out[n++] = (char)(ch + 0x20u);
    }
    for (; n < 7; n++) out[n] = 0;
}
// Header::parse (il2p_deframer.rs:289-319) on raw[0 .. 13); the record's pos, stream and diffs are the caller's
RR_IL2P_HD void il2p_parse(const unsigned char* d, Il2pRec* r) {
    il2p_callsign(d, r->dst);
    il2p_callsign(d + 6, r->src);
    r->dst_ssid = (unsigned char)(d[12] >> 4);
    r->src_ssid = (unsigned char)(d[12] & 0xf);
    r->flags = (unsigned char)((d[0] & 0x40 ? 1 : 0) | (d[0] & 0x80 ? 2 : 0) | (d[1] & 0x80 ? 4 : 0));
    r->pid = (unsigned char)(((d[1] & 0x40) >> 3) | ((d[2] & 0x40) >> 4) | ((d[3] & 0x40) >> 5) | ((d[4] & 0x40) >> 6));
    unsigned c = 0, ps = 0;
    for (int i = 0; i < 7; i++) c |= (unsigned)(d[5 + i] & 0x40) >> i;
    for (int i = 0; i < 10; i++) ps |= (unsigned)(d[2 + i] >> 7) << (9 - i);
    r->control = (unsigned char)c;
    r->payload_size = (unsigned short)ps;
}
// The whole record of the tag at virtual position v of the virtual stream W (readable one word beyond the header's last bit)
RR_IL2P_HD Il2pRec il2p_record(const il2p_u64* W, long v, unsigned long long pos, unsigned stream) {
    Il2pRec r{};
    r.pos = pos;
    r.stream = stream;
    {   // the tag's window with its oldest bit in bit 0: reversed into IL2P_SYNC's order
        const unsigned w = (unsigned)(il2p_win(W, v - 23) & 0xffffffull);
        unsigned rv = 0;
        for (int k = 0; k < IL2P_SYNC_BITS; k++) rv |= (w >> k & 1u) << (IL2P_SYNC_BITS - 1 - k);
        r.diffs = (unsigned char)__builtin_popcount(rv ^ IL2P_SYNC);
    }
    il2p_u64 y0, y1;
    il2p_descramble(il2p_win(W, v + 1), il2p_win(W, v + 65), &y0, &y1);
    il2p_header_bytes(y0, y1, r.raw);
    il2p_parse(r.raw, &r);
    return r;
}

}  // namespace rr
