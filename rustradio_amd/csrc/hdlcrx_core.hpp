// hdlcrx_core.hpp — the bit chain of rr_hdlc_receiver in word form: plain functions, no HIP types, shared by the
// mark stage of kernels_hdlcrx.hip and tests/cpp/emu_hdlcrx.cpp, which holds them to the bit-serial NrziDecode (src/nrzi.rs:36-41)
// and Descrambler (src/descrambler.rs:34-39) under g++.
// A stream's symbols of a push stand at the virtual positions C, C + 1, .. of its deframer (hdlc_core.hpp: C carried bits in front),
// so the chain runs in VIRTUAL coordinates: bit v of a word array is bit v & 63 of word v >> 6, symbol i is v = C + i.
//   R  the sliced (and inverted) symbols; r[-1], carried, stands at v = C - 1, everything else in front of C is 0
//   D  after NRZI: d[i] = 1 ^ r[i] ^ r[i - 1]; in front of C the 64 carried d[-64 .. -1] (RX_ST_DHIST), placed by rx_patch_d
//   S  after the descrambler: s[i] = d[i] ^ XOR d[i - delta] over the set bits (delta - 1) of dmask — each delay is one shifted word
// Nothing reaches back more than 65 bits, so two words of history in front of a tile are enough.
#pragma once
#include "hdlc_core.hpp"

namespace rr {

// a stream's state between pushes in front of the deframer's own (HdlcState): RX_ST_N words per stream
enum { RX_ST_RLAST = 0,                       // r[-1]: the last sliced (and inverted) symbol; 0 at the start (nrzi.rs:32-33)
       RX_ST_DHIST = 1,                       // bit 63 - k = d[-1 - k]: the last 64 bits in front of the descrambler
       RX_ST_POS = 2,                         // symbols of the stream so far
       RX_ST_N = 3 };

// Descrambler::new(mask, seed, len): shift_reg holds d[n - 1 - k] in bit len - k (descrambler.rs:37), so mask bit j reads
// d[n - delta], delta = 1 + len - j; before the stream the register is the seed.  len < 64 (bits_check).
RR_HDLC_HD hdlc_u64 rx_dmask(hdlc_u64 mask, unsigned len) {
    hdlc_u64 dm = 0;
    for (unsigned j = 0; j <= len; j++)
        if (mask >> j & 1ull) dm |= 1ull << (len - j);
    return dm;
}
RR_HDLC_HD hdlc_u64 rx_dhist0(hdlc_u64 seed, unsigned len) { return seed << (63 - len); }

// the bits of the word at virtual position vb that lie in front of virtual position k
RR_HDLC_HD hdlc_u64 rx_below(long vb, long k) {
    const long d = k - vb;
    return d <= 0 ? 0ull : d >= 64 ? ~0ull : (1ull << d) - 1ull;
}
// what of the 64 bits h, which stand at the virtual positions at .. at + 63, falls into the word at vb
RR_HDLC_HD hdlc_u64 rx_place(hdlc_u64 h, long at, long vb) {
    const long sh = at - vb;
    if (sh <= -64 || sh >= 64) return 0ull;
    return sh >= 0 ? h << sh : h >> -sh;
}
// NRZI on the word r0 with the word r1 in front of it (only its top bit is read)
RR_HDLC_HD hdlc_u64 rx_nrzi_word(hdlc_u64 r0, hdlc_u64 r1, bool nrzi) { return nrzi ? ~(r0 ^ (r0 << 1 | r1 >> 63)) : r0; }
// the D word at vb: its bits in front of C are the carried ones
RR_HDLC_HD hdlc_u64 rx_patch_d(hdlc_u64 d, long vb, long C, hdlc_u64 dhist) {
    const hdlc_u64 m = rx_below(vb, C);
    return (d & ~m) | (rx_place(dhist, C - 64, vb) & m);
}
// the descrambler on the D word cur with the D word prev in front of it
RR_HDLC_HD hdlc_u64 rx_descramble_word(hdlc_u64 cur, hdlc_u64 prev, hdlc_u64 dmask) {
    hdlc_u64 acc = cur;
    for (hdlc_u64 dm = dmask; dm; dm &= dm - 1) {
        const int delta = hdlc_ctz(dm) + 1;
        acc ^= delta == 64 ? prev : (cur << delta | prev >> (64 - delta));
    }
    return acc;
}
// the 64 bits of A that end at bit position p (p >= 63): bit 63 of the result is bit p
RR_HDLC_HD hdlc_u64 rx_win64(const hdlc_u64* A, long p) {
    const long b = p - 63, wi = b >> 6, off = b & 63;
    return off ? (A[wi] >> off) | (A[wi + 1] << (64 - off)) : A[wi];
}
// the decoded word at vb: S where the push's own bits C <= v < nv stand, the carried (already decoded) bits in front of them
RR_HDLC_HD hdlc_u64 rx_final_word(hdlc_u64 s, hdlc_u64 carried, long vb, long C, long nv) {
    return (s & ~rx_below(vb, C) & rx_below(vb, nv)) | (carried & rx_below(vb, C));
}

}  // namespace rr
