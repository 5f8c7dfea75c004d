// frame_core.hpp — the arithmetic the kernels of kernels_frame.hip share with the host: plain functions, no HIP types, so
// tests/test_frame_cpu.py compiles them with g++ and holds them to the reference's sequential loops.
//   StuffSum      the bit-stuffing counter of hdlc_encode (src/hdlc_framer.rs:65-80) as an associative summary
//   crc16_*       CRC-16/X.25 (calc_crc, src/hdlc_deframer.rs:309-315) of chunks and their combination
//   line_*        Scrambler::g3ruh (src/descrambler.rs:41-47) and NrziEncode (src/nrzi.rs:63-69) as one affine system over GF(2)
#pragma once
#if defined(__HIPCC__)
#define RR_FRAME_HD __host__ __device__ inline
#else
#define RR_FRAME_HD inline
#endif

namespace rr {

typedef unsigned long long frame_u64;

// ---- stuffing --------------------------------------------------------------------------------------------------------------------------
// A string of payload bits with packet starts between them.  A BREAK is a 0 bit or a packet start: the counter `ones` is 0
// behind it.  brk: the string holds a break; lead: the ones in front of the first break (the whole length without one);
// trail: the ones behind the last break modulo 5 (lead % 5 without one); stuffs: the stuffed bits of every run that begins
// behind a break — those of the leading run depend on what came before and are not counted.
struct StuffSum {
    unsigned brk, lead, trail, stuffs;
};
RR_FRAME_HD StuffSum stuff_none() { return StuffSum{0u, 0u, 0u, 0u}; }
RR_FRAME_HD StuffSum stuff_start() { return StuffSum{1u, 0u, 0u, 0u}; }                      // a packet start
RR_FRAME_HD StuffSum stuff_carry(unsigned ones) { return StuffSum{1u, 0u, ones % 5u, 0u}; }  // `ones` consecutive ones so far
RR_FRAME_HD StuffSum stuff_bit(unsigned b) { return b ? StuffSum{0u, 1u, 1u, 0u} : StuffSum{1u, 0u, 0u, 0u}; }
// a, then b
RR_FRAME_HD StuffSum stuff_combine(const StuffSum& a, const StuffSum& b) {
    StuffSum r;
    if (!a.brk) {
        r.brk = b.brk;
        r.lead = a.lead + b.lead;
        r.trail = b.brk ? b.trail : r.lead % 5u;
        r.stuffs = b.stuffs;
    } else {
        const unsigned j = a.trail + b.lead;          // the run that crosses the seam
        r.brk = 1u;
        r.lead = a.lead;
        r.trail = b.brk ? b.trail : j % 5u;
        r.stuffs = a.stuffs + j / 5u + b.stuffs;
    }
    return r;
}
// the 8 bits of a byte, LSB first
RR_FRAME_HD StuffSum stuff_byte(unsigned byte) {
    StuffSum s = stuff_none();
    for (int i = 0; i < 8; ++i) s = stuff_combine(s, stuff_bit(byte >> i & 1u));
    return s;
}

// ---- CRC-16/X.25 -----------------------------------------------------------------------------------------------------------------------
// Reflected: bit 15 of a word is x^0.  init == xorout == 0xffff, so crc(A ++ B) = x^(8 |B|) crc(A) ^ crc(B) in GF(2)[x] / P.
constexpr unsigned CRC16_POLY = 0x8408u;
RR_FRAME_HD unsigned crc16_byte(unsigned fcs, unsigned byte) {       // one step of the table-driven loop, without the table
    fcs ^= byte & 0xffu;
    for (int i = 0; i < 8; ++i) fcs = (fcs >> 1) ^ ((fcs & 1u) ? CRC16_POLY : 0u);
    return fcs;
}
RR_FRAME_HD unsigned crc16_mul(unsigned a, unsigned b) {             // a b mod P
    unsigned p = 0;
    for (unsigned m = 0x8000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC16_POLY : b >> 1;
    }
    return p;
}
RR_FRAME_HD unsigned crc16_xpow8(frame_u64 nbytes) {                 // x^(8 nbytes) mod P
    unsigned r = 0x8000u, sq = 0x0080u;                              // 1; x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1ull) r = crc16_mul(r, sq);
        sq = crc16_mul(sq, sq);
    }
    return r;
}

// ---- the line coder ------------------------------------------------------------------------------------------------------------------
// State word: bit k (k < 17) = s[n - 17 + k], the scrambler's register as descrambler.rs keeps it; bit 17 = NrziEncode's level.
constexpr int LINE_SCR = 1, LINE_NRZI = 2;
constexpr int LINE_T = 4096;                  // bits of one tile
constexpr int LINE_W = LINE_T / 64;
constexpr int LINE_K = 9;                     // 12 * 2^9 >= LINE_T: rounds of the zero-state response
constexpr int LINE_NS = 18;                   // bits of the state
constexpr int LINE_NP = 20;                   // powers M^(2^r), r < LINE_NP
static_assert((12 << LINE_K) >= LINE_T && (12 << (LINE_K - 1)) < LINE_T, "LINE_K = ceil(log2(LINE_T / 12))");

// one step of the reference's two blocks on the state word -> the output bit
RR_FRAME_HD unsigned line_step(unsigned& st, unsigned in, int mode) {
    unsigned o = in & 1u;
    if (mode & LINE_SCR) {
        const unsigned reg = st & 0x1ffffu;
        o = reg & 1u;                                                  // next_scramble: ret = shift_reg & 1
        const unsigned tmp = ((reg >> 5) ^ reg ^ in) & 1u;             // mask 0x21
        st = (st & ~0x1ffffu) | (reg >> 1) | (tmp << 16);
    }
    if (mode & LINE_NRZI) {
        if (!o) st ^= 1u << 17;
        o = st >> 17 & 1u;
    }
    return o;
}
// word w of the array a (nw words, bit n of the stream = bit n & 63 of word n >> 6) delayed by d bits; zeros come in
RR_FRAME_HD frame_u64 line_delay(const frame_u64* a, int w, int d) {
    const int q = d >> 6, r = d & 63;
    const frame_u64 hi = w - q >= 0 ? a[w - q] : 0ull, lo = w - q - 1 >= 0 ? a[w - q - 1] : 0ull;
    return r ? (hi << r) | (lo >> (64 - r)) : hi;
}
// what the register `reg` of the previous tile adds to the first word of this tile's input: s[n - 12] for n < 12 and s[n - 17]
// for n < 17 are bits of the register
RR_FRAME_HD frame_u64 line_inject(unsigned reg) {
    reg &= 0x1ffffu;
    return (frame_u64)(reg >> 5) ^ (frame_u64)reg;                     // bit n: reg bit (n + 5), n < 12; reg bit n, n < 17
}
// y = M x: row i of M in m[i]
RR_FRAME_HD unsigned line_matvec(const unsigned* m, unsigned x) {
    unsigned y = 0;
    for (int i = 0; i < LINE_NS; ++i) {
        y |= ((unsigned)__builtin_popcount(m[i] & x) & 1u) << i;
    }
    return y;
}
// M^len x from the table of M^(2^r)
RR_FRAME_HD unsigned line_pow_apply(const unsigned* pw, frame_u64 len, unsigned x) {
    for (int r = 0; len && r < LINE_NP; ++r, len >>= 1)
        if (len & 1ull) x = line_matvec(pw + r * LINE_NS, x);
    return x;
}

// ---- host only ----
// pw[r] = M^(2^r), M = the linear part of LINE_T steps with zero input (the constant part is in every tile's z)
inline void line_build_powers(int mode, unsigned* pw) {
    unsigned zero = 0;
    for (int t = 0; t < LINE_T; ++t) line_step(zero, 0u, mode);         // the affine part: what the zero state becomes
    unsigned col[LINE_NS];
    for (int j = 0; j < LINE_NS; ++j) {
        unsigned st = 1u << j;
        for (int t = 0; t < LINE_T; ++t) line_step(st, 0u, mode);
        col[j] = st ^ zero;
    }
    for (int i = 0; i < LINE_NS; ++i) {
        unsigned row = 0;
        for (int j = 0; j < LINE_NS; ++j) row |= (col[j] >> i & 1u) << j;
        pw[i] = row;
    }
    for (int r = 1; r < LINE_NP; ++r) {                                // square: row i of A A = XOR of A's rows j over the bits j of row i
        const unsigned* a = pw + (r - 1) * LINE_NS;
        unsigned* b = pw + r * LINE_NS;
        for (int i = 0; i < LINE_NS; ++i) {
            unsigned row = 0;
            for (int j = 0; j < LINE_NS; ++j)
                if (a[i] >> j & 1u) row ^= a[j];
            b[i] = row;
        }
    }
}
// One whole tile from the zero state, as the kernels compute it: in -> the state it leaves (z) and, with `out`, its output
// words.  st_in: the state in front of the tile (0 for z).
inline unsigned line_tile_words(const frame_u64* in, int mode, unsigned st_in, frame_u64* out) {
    frame_u64 a[LINE_W], b[LINE_W];
    for (int w = 0; w < LINE_W; ++w) a[w] = in[w];
    unsigned st = 0;
    if (mode & LINE_SCR) {
        a[0] ^= line_inject(st_in);
        for (int k = 0; k < LINE_K; ++k) {
            for (int w = 0; w < LINE_W; ++w) b[w] = a[w] ^ line_delay(a, w, 12 << k) ^ line_delay(a, w, 17 << k);
            for (int w = 0; w < LINE_W; ++w) a[w] = b[w];
        }
        st = (unsigned)(a[LINE_W - 1] >> 47);                          // the last 17 bits of s
        for (int w = 0; w < LINE_W; ++w) b[w] = line_delay(a, w, 17);  // out[n] = s[n - 17]
        b[0] |= (frame_u64)(st_in & 0x1ffffu);
        for (int w = 0; w < LINE_W; ++w) a[w] = b[w];
    }
    if (mode & LINE_NRZI) {
        unsigned lvl = st_in >> 17 & 1u;
        for (int w = 0; w < LINE_W; ++w) {
            frame_u64 x = ~a[w];
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
            if (lvl) x = ~x;
            a[w] = x;
            lvl = (unsigned)(x >> 63);
        }
        st |= lvl << 17;
    }
    if (out)
        for (int w = 0; w < LINE_W; ++w) out[w] = a[w];
    return st;
}

}  // namespace rr
