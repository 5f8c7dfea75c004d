// emu_frame.cpp — the arithmetic of rustradio_amd/csrc/frame_core.hpp on the CPU, against the reference's sequential loops written
// out here (no HIP; built by tests/test_frame_cpu.py with g++):
//   1. the stuffing summary and its combine, exhaustively: every bit string of up to 14 bits, cut at every point, with and without
//      a packet start at the cut, from every value of the counter, against hdlc_encode's counter (src/hdlc_framer.rs:65-80)
//   2. CRC chunks combined by x^(8 len) against calc_crc's loop (src/hdlc_deframer.rs:309-315)
//   3. the tile recurrence c' = M c ^ z and the tile's words against the Lfsr (src/descrambler.rs:41-47) and NrziEncode
//      (src/nrzi.rs:63-69) run bit by bit, 1,000 random tiles per mode, and chains of tiles through the powers of M
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "frame_core.hpp"

using namespace rr;

static int fails = 0;
#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                          \
    } while (0)

// hdlc_encode's counter over bits[lo, hi) from `ones`; a packet start (start_at == position) resets it -> stuffed bits
static unsigned seq_stuff(unsigned bits, int lo, int hi, int start_at, unsigned& ones) {
    unsigned stuffed = 0;
    for (int i = lo; i < hi; i++) {
        if (i == start_at) ones = 0;
        if (bits >> i & 1u) {
            if (++ones == 5) { ones = 0; stuffed++; }
        } else {
            ones = 0;
        }
    }
    if (hi == start_at) ones = 0;
    return stuffed;
}
static StuffSum fold(unsigned bits, int lo, int hi) {
    StuffSum s = stuff_none();
    for (int i = lo; i < hi; i++) s = stuff_combine(s, stuff_bit(bits >> i & 1u));
    return s;
}
static void test_stuffing() {
    long cases = 0;
    for (int n = 0; n <= 14; n++)
        for (unsigned bits = 0; bits < (1u << n); bits++)
            for (int cut = 0; cut <= n; cut++)
                for (int with_start = 0; with_start < 2; with_start++) {
                    StuffSum a = fold(bits, 0, cut), b = fold(bits, cut, n);
                    if (with_start) b = stuff_combine(stuff_start(), b);
                    const StuffSum ab = stuff_combine(a, b);
                    for (unsigned c = 0; c < 5; c++) {
                        unsigned ones = c;
                        const unsigned want = seq_stuff(bits, 0, n, with_start ? cut : -1, ones);
                        const StuffSum r = stuff_combine(stuff_carry(c), ab);
                        CHECK(r.brk == 1 && r.stuffs == want && r.trail == ones, "n %d bits %x cut %d start %d c %u: %u/%u want %u/%u", n, bits, cut,
                              with_start, c, r.stuffs, r.trail, want, ones);
                        cases++;
                    }
                    // associativity with a third piece in front: (x a) b == x (a b)
                    const StuffSum x = stuff_byte(bits & 0xffu);
                    const StuffSum l = stuff_combine(stuff_combine(x, a), b), r2 = stuff_combine(x, ab);
                    CHECK(l.brk == r2.brk && l.lead == r2.lead && l.trail == r2.trail && l.stuffs == r2.stuffs, "associativity n %d bits %x cut %d", n,
                          bits, cut);
                }
    // a run without a break longer than several tiles: lead carries the whole length
    StuffSum t = stuff_none();
    for (int i = 0; i < 3 * 4096 + 8; i++) t = stuff_combine(t, stuff_bit(1));
    CHECK(!t.brk && t.lead == 3 * 4096 + 8 && t.stuffs == 0, "all ones");
    const StuffSum r = stuff_combine(stuff_start(), t);
    CHECK(r.stuffs == (3 * 4096 + 8) / 5 && r.trail == (3 * 4096 + 8) % 5, "all ones behind a start");
    std::printf("stuffing: %ld cases\n", cases);
}

static unsigned crc_ref(const unsigned char* d, size_t n) {       // calc_crc with the table of RFC 1662 built from its generator
    static unsigned tab[256];
    static bool init = false;
    if (!init) {
        for (unsigned b = 0; b < 256; b++) {
            unsigned v = b;
            for (int i = 0; i < 8; i++) v = v & 1 ? (v >> 1) ^ 0x8408u : v >> 1;
            tab[b] = v;
        }
        init = true;
    }
    unsigned fcs = 0xffffu;
    for (size_t i = 0; i < n; i++) fcs = (fcs >> 8) ^ tab[(fcs ^ d[i]) & 0xffu];
    return fcs ^ 0xffffu;
}
static void test_crc(std::mt19937& rng) {
    const unsigned char hello[] = {0x82, 0xa0, 0xb4, 0x60, 0x60, 0x62, 0x60, 0x9a, 0x60, 0xa8, 0x90, 0x86, 0x40, 0xe5, 0x03, 0xf0, 0x3a,
                                   0x4d, 0x30, 0x54, 0x48, 0x43, 0x2d, 0x31, 0x20, 0x20, 0x3a, 0x68, 0x65, 0x6c, 0x6c, 0x6f, 0x41};
    CHECK(crc_ref(hello, sizeof hello) == 0xdc7du, "the fcs vector");
    for (int it = 0; it < 400; it++) {
        const size_t n = rng() % 3000, chunk = 1 + rng() % 300;
        std::vector<unsigned char> d(n);
        for (auto& v : d) v = (unsigned char)rng();
        unsigned x = 0;
        for (size_t b0 = 0; b0 < n; b0 += chunk) {
            const size_t b1 = std::min(n, b0 + chunk);
            unsigned fcs = 0xffffu;
            for (size_t i = b0; i < b1; i++) fcs = crc16_byte(fcs, d[i]);
            x ^= crc16_mul(crc16_xpow8(n - b1), fcs ^ 0xffffu);
        }
        CHECK(x == crc_ref(d.data(), n), "crc n %zu chunk %zu", n, chunk);
    }
}

// the reference's two blocks, bit by bit
struct RefLine {
    uint64_t shift_reg = 0;
    unsigned out = 0;
    int mode;
    unsigned step(unsigned i) {
        unsigned o = i;
        if (mode & LINE_SCR) {
            o = (unsigned)(shift_reg & 1);
            const unsigned tmp = 1u & ((unsigned)__builtin_popcountll(shift_reg & 0x21) ^ i);
            shift_reg = (shift_reg >> 1) | ((uint64_t)tmp << 16);
        }
        if (mode & LINE_NRZI) {
            if (o == 0) out ^= 1;
            o = out;
        }
        return o;
    }
    unsigned state() const { return (mode & LINE_SCR ? (unsigned)shift_reg : 0u) | (mode & LINE_NRZI ? out << 17 : 0u); }
    void set(unsigned st) { shift_reg = mode & LINE_SCR ? st & 0x1ffffu : 0; out = mode & LINE_NRZI ? st >> 17 & 1u : 0; }
};
static void test_line(std::mt19937& rng) {
    for (int mode = 1; mode <= 3; mode++) {
        std::vector<unsigned> pw(LINE_NP * LINE_NS);
        line_build_powers(mode, pw.data());
        const unsigned live = (mode & LINE_SCR ? 0x1ffffu : 0u) | (mode & LINE_NRZI ? 1u << 17 : 0u);
        for (int it = 0; it < 1000; it++) {
            frame_u64 in[LINE_W], out[LINE_W];
            const int kind = it % 4;                              // random, sparse, all ones, all zeros
            for (auto& w : in) {
                const frame_u64 r = (frame_u64)rng() << 32 | rng();
                w = kind == 0 ? r : kind == 1 ? r & ((frame_u64)rng() << 32 | rng()) & ((frame_u64)rng() << 32 | rng()) : kind == 2 ? ~0ull : 0ull;
            }
            const unsigned c = rng() & live;
            RefLine ref{};
            ref.mode = mode;
            ref.set(c);
            bool same = true;
            for (int n = 0; n < LINE_T; n++) ref.step((unsigned)(in[n >> 6] >> (n & 63)) & 1u);
            const unsigned z = line_tile_words(in, mode, 0u, nullptr);
            CHECK((line_matvec(pw.data(), c) ^ z) == ref.state(), "mode %d tile %d: M c ^ z = %x, the register holds %x", mode, it,
                  line_matvec(pw.data(), c) ^ z, ref.state());
            const unsigned st = line_tile_words(in, mode, c, out);
            CHECK(st == ref.state(), "mode %d tile %d: state %x want %x", mode, it, st, ref.state());
            ref.set(c);
            for (int n = 0; n < LINE_T && same; n++)
                same = ref.step((unsigned)(in[n >> 6] >> (n & 63)) & 1u) == ((unsigned)(out[n >> 6] >> (n & 63)) & 1u);
            CHECK(same, "mode %d tile %d: output bits", mode, it);
        }
        // chains: the state behind T tiles through the powers of M, as k_line_scan forms it
        for (int it = 0; it < 20; it++) {
            const int T = 1 + (int)(rng() % 200);
            std::vector<frame_u64> in((size_t)T * LINE_W);
            for (auto& w : in) w = (frame_u64)rng() << 32 | rng();
            const unsigned c0 = rng() & live;
            RefLine ref{};
            ref.mode = mode;
            ref.set(c0);
            unsigned acc = 0;                                     // sum of M^(T-1-t) z_t
            for (int t = 0; t < T; t++) {
                for (int n = 0; n < LINE_T; n++) ref.step((unsigned)(in[(size_t)t * LINE_W + (n >> 6)] >> (n & 63)) & 1u);
                acc = line_matvec(pw.data(), acc) ^ line_tile_words(in.data() + (size_t)t * LINE_W, mode, 0u, nullptr);
            }
            CHECK((line_pow_apply(pw.data(), (frame_u64)T, c0) ^ acc) == ref.state(), "mode %d chain of %d tiles", mode, T);
        }
    }
}

int main() {
    std::mt19937 rng(12345);
    test_stuffing();
    test_crc(rng);
    test_line(rng);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("frame core ok\n");
    return 0;
}
