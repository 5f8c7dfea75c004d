// kiss_core.hpp — the arithmetic the kernels of kernels_kiss.hip share with the host: plain functions, no HIP types, so
// tests/cpp/emu_kiss.cpp compiles them with g++ and holds them to tests/kiss_model.py.
//   KissSum       what a string of bytes leaves behind for the bytes after it, as an associative summary
//   kiss_close    KissFrame (src/kiss.rs:165-228) -> KissDecode (:96-137) for the gap a FEND closes, from the summary in front of it
//   kiss_next     what a push carries into the next one
//   kiss_escapes  escape (src/kiss.rs:30-44) per byte
#pragma once
#if defined(__HIPCC__)
#define RR_KISS_HD __host__ __device__ inline
#else
#define RR_KISS_HD inline
#endif

namespace rr {

constexpr unsigned KISS_FEND = 0xC0, KISS_FESC = 0xDB, KISS_TFEND = 0xDC, KISS_TFESC = 0xDD;      // src/kiss.rs:7-10
constexpr int KISS_T = 4096;                  // bytes of a tile: 256 threads of 16
constexpr int KISS_LANE = 16;                 // bytes of a thread

// KissSum::last when it is no index of the push's virtual stream (carried bytes, then the window):
constexpr int KISS_VIRT = -1;                 // the FEND in front of the carried bytes (Synced(v), v = the carried bytes)
constexpr int KISS_UNSYNC = -2;               // no FEND yet (Unsynced at the start of the stream)
constexpr int KISS_OVER = -3;                 // a FEND, and more than max_len bytes behind it (Unsynced, :216-217; its FEND counts the gap)
constexpr int KISS_NONE = -4;                 // the string holds no FEND: what was in front of it stands

// nesc / nbad / nfend: the FESC bytes, the bad escapes and the FENDs of the string.  A bad escape is a FESC whose next byte
// exists and is neither TFEND nor TFESC (unescape, :47-77: "invalid escape byte", "ended on an escape" when the next is the
// closing FEND).  last: the index of its last FEND; el / bl: the FESC bytes and bad escapes in front of that FEND.
struct KissSum {
    unsigned nesc, nbad, nfend;
    int last;
    unsigned el, bl;
};
RR_KISS_HD KissSum kiss_none() { return KissSum{0u, 0u, 0u, KISS_NONE, 0u, 0u}; }
RR_KISS_HD KissSum kiss_seed(int code) { return KissSum{0u, 0u, 0u, code, 0u, 0u}; }       // what the stream so far left behind
// a, then b
RR_KISS_HD KissSum kiss_combine(const KissSum& a, const KissSum& b) {
    KissSum r;
    r.nesc = a.nesc + b.nesc;
    r.nbad = a.nbad + b.nbad;
    r.nfend = a.nfend + b.nfend;
    if (b.last != KISS_NONE) { r.last = b.last; r.el = a.nesc + b.el; r.bl = a.nbad + b.bl; }
    else { r.last = a.last; r.el = a.el; r.bl = a.bl; }
    return r;
}
// the byte at index v; has_next: a byte follows it in the virtual stream
RR_KISS_HD KissSum kiss_byte(int v, unsigned cur, unsigned next, bool has_next) {
    if (cur == KISS_FEND) return KissSum{0u, 0u, 1u, v, 0u, 0u};
    if (cur == KISS_FESC) return KissSum{1u, has_next && next != KISS_TFEND && next != KISS_TFESC ? 1u : 0u, 0u, KISS_NONE, 0u, 0u};
    return kiss_none();
}

// The gap a FEND at index e closes, `run` being the summary of everything in front of e.
enum { KISS_G_NOTHING = 0, KISS_G_DELIVERED = 1, KISS_G_NONDATA = 2, KISS_G_BADESC = 3, KISS_G_OVERLONG = 4 };
struct KissGap {
    int kind;
    unsigned port, in_bytes, len;             // of a delivered packet
};
// the length of that gap, or -1: there is none (no FEND in front), -2: it is over-long whatever follows
RR_KISS_HD long kiss_gap_len(const KissSum& run, int e) {
    if (run.last == KISS_UNSYNC || run.last == KISS_NONE) return -1;
    if (run.last == KISS_OVER) return -2;
    return (long)e - (long)run.last - 1;
}
// port_byte: the gap's first byte (asked for only when 1 <= length <= max_len)
RR_KISS_HD KissGap kiss_close(const KissSum& run, long glen, unsigned max_len, unsigned port_byte) {
    KissGap g{KISS_G_NOTHING, 0u, 0u, 0u};
    if (glen == -2 || glen > (long)max_len) { g.kind = KISS_G_OVERLONG; return g; }
    if (glen <= 0) return g;                                                  // (strip_fend, :105-108)
    if (port_byte & 0xFu) { g.kind = KISS_G_NONDATA; return g; }             // (:110-113)
    // a data port byte is no FESC, so the FESC bytes and bad escapes since the opening FEND are those of x = G[1..]
    if (run.nbad != run.bl) { g.kind = KISS_G_BADESC; return g; }
    g.kind = KISS_G_DELIVERED;
    g.port = port_byte >> 4;
    g.in_bytes = (unsigned)(glen - 1);
    g.len = g.in_bytes - (run.nesc - run.el);
    return g;
}
// A byte of x at index v of a delivered gap: false when it is a FESC (it stores nothing); else its rank in the packet and its value.
RR_KISS_HD bool kiss_emit(const KissSum& run, int v, unsigned prev, unsigned cur, unsigned* rank, unsigned* value) {
    const long j = (long)v - (long)run.last - 2;                              // its place in x
    if (j < 0 || cur == KISS_FESC) return false;
    *rank = (unsigned)j - (run.nesc - run.el);
    const bool esc = j > 0 && prev == KISS_FESC;
    *value = esc ? (cur == KISS_TFEND ? KISS_FEND : KISS_FESC) : cur;         // (a delivered gap holds no other escape)
    return true;
}
// What a push of `len` virtual bytes with the summary `root` carries on: *code = KISS_VIRT with *carry bytes (the last ones of
// the virtual stream), or KISS_UNSYNC / KISS_OVER with none.
RR_KISS_HD void kiss_next(const KissSum& root, long len, unsigned max_len, int* code, unsigned* carry) {
    *carry = 0;
    if (root.last == KISS_UNSYNC || root.last == KISS_OVER || root.last == KISS_NONE) { *code = root.last == KISS_OVER ? KISS_OVER : KISS_UNSYNC; return; }
    const long open = len - (long)root.last - 1;
    if (open > (long)max_len) { *code = KISS_OVER; return; }
    *code = KISS_VIRT;
    *carry = (unsigned)open;
}

// escape (src/kiss.rs:35-41): the bytes a payload byte adds to its own
RR_KISS_HD unsigned kiss_escapes(unsigned b) { return b == KISS_FEND || b == KISS_FESC ? 1u : 0u; }
// KissEncode's port (src/kiss.rs:256-266): a port of 16 or more is 0
RR_KISS_HD unsigned kiss_port_byte(unsigned long long port) { return port < 16 ? (unsigned)(port << 4) & 0xFFu : 0u; }

}  // namespace rr
