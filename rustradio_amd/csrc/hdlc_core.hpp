// hdlc_core.hpp — the arithmetic the kernels of kernels_hdlc.hip share with the host: plain functions, no HIP types, so
// tests/cpp/emu_hdlc.cpp compiles them with g++ and holds them to the reference's sequential machine.
// HdlcDeframer (src/hdlc_deframer.rs:123-232) in the flag-to-flag formulation of tests/hdlc_model.py deframe_events:
//   hdlc_marks      flag ends, aborts (the seventh 1) and stuffed zeros of 64 bits at once
//   hdlc_map_*      one map over {S, U, U3} per gap between two flag ends, and its composition
//   hdlc_gap_scan   the map of one gap and the bits it keeps
//   hdlc_select / hdlc_take_byte      destuffing: where kept bit k of a gap lies, and the byte that starts there
//   hdlc_crc_part / hdlc_syn_*        CRC-16/X.25 by chunks (frame_core.hpp's crc16_*) and the single-bit repair as a syndrome search
//   hdlc_carry_plan what of the virtual stream the next push has to see again
// The bits of a push stand behind what the previous push left (8 halo bits, then the raw bits of the gap still open): the
// VIRTUAL stream.  Bit v of it is bit v & 63 of word v >> 6.
#pragma once
#include "frame_core.hpp"

#define RR_HDLC_HD RR_FRAME_HD

namespace rr {

typedef unsigned long long hdlc_u64;

// The machine at a flag end (the ANCHOR).  S: Synced with nothing collected.  U: Unsynced, and every later flag is seen whole.
// U3: Unsynced since this very bit (FinalCheck with fewer than 7 bits, hdlc_deframer.rs:173-176): a flag that ends 7 bits on is not seen.
constexpr int HDLC_S = 0, HDLC_U = 1, HDLC_U3 = 2;
constexpr int HDLC_HALO = 8;                  // bits in front of the carried gap: the anchor's flag, or 8 bits nobody asks about

RR_HDLC_HD int hdlc_popc(hdlc_u64 x) { return __builtin_popcountll(x); }
RR_HDLC_HD int hdlc_ctz(hdlc_u64 x) { return __builtin_ctzll(x); }

// ---- the local features -------------------------------------------------------------------------------------------------------------
struct HdlcMarks {
    hdlc_u64 flag, abort, stuffed;
};
// cur: 64 bits of the stream, prev: the 64 in front of them (only its top 7 bits are read)
RR_HDLC_HD HdlcMarks hdlc_marks(hdlc_u64 cur, hdlc_u64 prev) {
    hdlc_u64 ones5 = ~0ull;
    for (int k = 1; k <= 5; ++k) ones5 &= (cur << k) | (prev >> (64 - k));
    const hdlc_u64 run6 = ones5 & ((cur << 6) | (prev >> 58)), back7 = (cur << 7) | (prev >> 57);
    HdlcMarks m;
    m.flag = ~cur & run6 & ~back7;            // 0 111111 0 ends here
    m.abort = cur & run6;                     // the seventh 1 in a row
    m.stuffed = ~cur & ones5 & ~run6;         // a 0 behind exactly five 1s
    return m;
}

// ---- the maps ---------------------------------------------------------------------------------------------------------------------------
// bits 2 i + 1 : 2 i = what state i at the gap's first flag end becomes at its second; HDLC_EMITS: entered in S, the gap is a frame
typedef unsigned hdlc_map;
constexpr hdlc_map HDLC_MAP_ID = 0u | 1u << 2 | 2u << 4, HDLC_MAP_MASK = 0x3fu, HDLC_EMITS = 0x40u;
RR_HDLC_HD hdlc_map hdlc_map_make(int from_s, int from_u, int from_u3) { return (hdlc_map)(from_s | from_u << 2 | from_u3 << 4); }
RR_HDLC_HD int hdlc_map_at(hdlc_map m, int st) { return (int)(m >> (2 * st)) & 3; }
// a, then b (the emit bit belongs to one gap and is dropped)
RR_HDLC_HD hdlc_map hdlc_map_then(hdlc_map a, hdlc_map b) {
    return hdlc_map_make(hdlc_map_at(b, hdlc_map_at(a, 0)), hdlc_map_at(b, hdlc_map_at(a, 1)), hdlc_map_at(b, hdlc_map_at(a, 2)));
}
// share: the second flag's first 0 is the first flag's last (f == s + 7).  reset: Synced gave up inside the gap (too long,
// hdlc_deframer.rs:144-146, or an abort, :173-176); hides: ... within the second flag's last 7 bits, so that flag is not seen whole.
RR_HDLC_HD hdlc_map hdlc_gap_map(bool share, bool reset, bool hides) {
    const int from_u3 = share ? HDLC_U : HDLC_S;
    if (reset) return hdlc_map_make(hides ? HDLC_U : HDLC_S, HDLC_S, from_u3);
    if (share) return hdlc_map_make(HDLC_U3, HDLC_S, from_u3);
    return hdlc_map_make(HDLC_S, HDLC_S, from_u3) | HDLC_EMITS;
}

// The raw bits behind a flag end within which `collected > 8 max_size` is certain: a stuffed bit needs five kept ones in front of
// it, so R raw bits keep at least R - floor(R / 6), and M = 8 max_size + 1 kept bits are reached by R = M + floor((M - 1) / 5)
// at the latest (all ones reach it exactly).  The reset itself happens on the bit behind them.
RR_HDLC_HD hdlc_u64 hdlc_reset_bits(hdlc_u64 max_size) {
    const hdlc_u64 m = 8 * max_size + 1;
    return m + (m - 1) / 5;
}
// A gap of more raw bits than this has reset more than 7 bits in front of its closing flag whatever it holds: it leaves S.
RR_HDLC_HD hdlc_u64 hdlc_reach(hdlc_u64 max_size) { return hdlc_reset_bits(max_size) + 8; }

struct HdlcGap {
    hdlc_map map;
    hdlc_u64 kept;                            // with HDLC_EMITS: the bits of the gap that are not stuffed, the closing flag's first 7 included
};
// The gap between the flag ends s < f: ab / st are the abort and stuffed masks of the virtual stream.
RR_HDLC_HD HdlcGap hdlc_gap_scan(const hdlc_u64* ab, const hdlc_u64* st, long s, long f, hdlc_u64 max_size) {
    HdlcGap g;
    g.kept = 0;
    const bool share = f == s + 7;
    if ((hdlc_u64)(f - 1 - s) > hdlc_reach(max_size)) { g.map = hdlc_gap_map(share, true, false); return g; }
    const hdlc_u64 maxbits = 8 * max_size;
    hdlc_u64 coll = 0;                        // collected in front of bit p
    long r = -1;
    for (long p = s + 1; p < f && r < 0;) {
        const long w = p >> 6, end = ((w + 1) << 6) < f ? ((w + 1) << 6) : f;      // this word's bits [p, end) of the gap
        const hdlc_u64 m = (~0ull << (p & 63)) & (end - (w << 6) == 64 ? ~0ull : (1ull << (end - (w << 6))) - 1ull);
        const hdlc_u64 a = ab[w] & m, stuffed = st[w] & m;
        // collected in front of the word's last bit: the reset looks at the count before it looks at the bit
        const hdlc_u64 last = coll + (hdlc_u64)(end - 1 - p) - (hdlc_u64)hdlc_popc(stuffed & ~(1ull << ((end - 1) & 63)));
        long over = -1;
        if (last > maxbits) {
            hdlc_u64 c = coll;
            for (long q = p; q < end; ++q) {
                if (c > maxbits) { over = q; break; }
                c += 1 - (stuffed >> (q & 63) & 1ull);
            }
        }
        const long abort = a ? (w << 6) + hdlc_ctz(a) : -1;
        if (over >= 0 && (abort < 0 || over < abort)) r = over;
        else if (abort >= 0) r = abort;
        coll += (hdlc_u64)(end - p) - (hdlc_u64)hdlc_popc(stuffed);
        p = end;
    }
    if (r >= 0) { g.map = hdlc_gap_map(share, true, r >= f - 7); return g; }
    g.map = hdlc_gap_map(share, false, false);
    g.kept = coll;
    return g;
}

// The bytes a gap of `kept` bits delivers (hdlc_deframer.rs:178-190), or -1: not a whole number of bytes, or fewer than min_size.
RR_HDLC_HD long hdlc_frame_bytes(hdlc_u64 kept, hdlc_u64 min_size) {
    if (kept < 7) return -1;                  // (a gap that emits holds the closing flag's first 7 bits)
    const hdlc_u64 bits = kept - 7;
    if (bits % 8 || bits / 8 < min_size) return -1;
    return (long)(bits / 8);
}

// ---- destuffing ---------------------------------------------------------------------------------------------------------------------
// the position of kept bit number k (from 0) behind s, or -1 if there are not that many in front of `end`
RR_HDLC_HD long hdlc_select(const hdlc_u64* st, long s, long end, hdlc_u64 k) {
    for (long p = s + 1; p < end;) {
        const long w = p >> 6;
        hdlc_u64 keep = ~st[w] & (~0ull << (p & 63));
        const hdlc_u64 c = (hdlc_u64)hdlc_popc(keep);
        if (k < c) {
            for (; k; --k) keep &= keep - 1;
            const long q = (w << 6) + hdlc_ctz(keep);
            return q < end ? q : -1;
        }
        k -= c;
        p = (w + 1) << 6;
    }
    return -1;
}
// a position with the two words under it, so that a walk loads each word once
struct HdlcCursor {
    long p, w;
    hdlc_u64 raw, st;
};
RR_HDLC_HD HdlcCursor hdlc_cursor(const hdlc_u64* raw, const hdlc_u64* st, long p) {
    HdlcCursor c;
    c.p = p; c.w = p >> 6; c.raw = raw[c.w]; c.st = st[c.w];
    return c;
}
// the byte whose lowest bit is the first kept bit at or behind c.p; c.p moves behind its highest bit
RR_HDLC_HD unsigned hdlc_take_byte(const hdlc_u64* raw, const hdlc_u64* st, HdlcCursor& c) {
    unsigned byte = 0;
    for (int i = 0; i < 8; ++c.p) {
        if ((c.p >> 6) != c.w) { c.w = c.p >> 6; c.raw = raw[c.w]; c.st = st[c.w]; }
        const int b = (int)(c.p & 63);
        if (c.st >> b & 1ull) continue;
        byte |= (unsigned)(c.raw >> b & 1ull) << i;
        ++i;
    }
    return byte;
}
// Where a lane of 64 starts looking for kept bit t of the gap behind s: the gap's words [wf, wf + 64 seg) are cut into 64
// segments of seg words, before[j] = the kept bits in front of segment j.  -> the j to pass to hdlc_seg_from; all 64 lanes
// run the same six steps, `at(j)` reads lane j's `before`.
template <class F> RR_HDLC_HD int hdlc_seg_find(hdlc_u64 t, F&& at) {
    int lo = 0, hi = 63;
    for (int step = 0; step < 6; ++step) {      // the last segment with before <= t
        const int mid = (lo + hi + 1) >> 1;
        const hdlc_u64 b = at(mid);
        if (lo < hi) { if (b <= t) lo = mid; else hi = mid - 1; }
    }
    return lo;
}
// the position in front of segment j's first bit (hdlc_select counts from the bit behind it)
RR_HDLC_HD long hdlc_seg_from(long s, long wf, long seg, int j) { return j ? ((wf + j * seg) << 6) - 1 : s; }

// ---- the checksum -------------------------------------------------------------------------------------------------------------------------
// a chunk's running fcs (from 0xffff, crc16_byte per byte) as its share of the whole CRC: `behind` bytes follow it
RR_HDLC_HD unsigned hdlc_crc_part(unsigned fcs, hdlc_u64 behind) { return crc16_mul(crc16_xpow8(behind), (fcs ^ 0xffffu) & 0xffffu); }

// Flipping the data bit d bits in front of the end of the data changes the CRC by syn(d), whatever the data:
// syn(0) = 0x0001, syn(d + 1) = step(syn(d)) (find_right_crc, hdlc_deframer.rs:41-71, as a search)
RR_HDLC_HD unsigned hdlc_syn_step(unsigned v) { return (v >> 1) ^ ((v & 1u) ? CRC16_POLY : 0u); }
RR_HDLC_HD unsigned hdlc_syn(hdlc_u64 d) {
    unsigned r = 0x8000u, sq = 0x4000u;       // 1; x
    for (; d; d >>= 1) {
        if (d & 1ull) r = crc16_mul(r, sq);
        sq = crc16_mul(sq, sq);
    }
    return crc16_mul(r, 0x0001u);
}
// the lowest bit h in [h0, h1) of nbits data bits whose flip changes the CRC by diff, or -1
RR_HDLC_HD long hdlc_syn_search(unsigned diff, hdlc_u64 nbits, hdlc_u64 h0, hdlc_u64 h1) {
    if (h0 >= h1) return -1;
    long hit = -1;
    unsigned v = hdlc_syn(nbits - h1);
    for (hdlc_u64 h = h1; h > h0; --h) {      // d = nbits - h + 1 upwards: the last hit is the lowest bit
        v = hdlc_syn_step(v);
        if (v == diff) hit = (long)(h - 1);
    }
    return hit;
}

// ---- the carry --------------------------------------------------------------------------------------------------------------------------
// What the next push sees in front of its bits: the virtual bits [from, from + count) and the state of the anchor, which is
// bit from + 7.  last_end: the last flag end of this push's virtual stream (HDLC_HALO - 1: none, the anchor it came with),
// state: the machine there, nv: the virtual bits.  A gap whose outcome no longer depends on its bits (state U, or longer than
// hdlc_reach: it leaves S, as U does) is cut down to the last 8 bits, which the features of the next bits look back at.
struct HdlcCarry {
    long from, count;
    int state;
};
RR_HDLC_HD HdlcCarry hdlc_carry_plan(long last_end, int state, long nv, hdlc_u64 max_size) {
    HdlcCarry c;
    const hdlc_u64 open = (hdlc_u64)(nv - 1 - last_end);
    if (state == HDLC_U || open > hdlc_reach(max_size)) {
        c.from = nv - HDLC_HALO; c.count = HDLC_HALO; c.state = HDLC_U;
    } else {
        c.from = last_end - (HDLC_HALO - 1); c.count = nv - c.from; c.state = state;
    }
    return c;
}

}  // namespace rr
