// emu_hdlcrx.cpp — the word-form bit chain of rustradio_amd/csrc/hdlcrx_core.hpp on the CPU, run thread by thread the way the mark
// stage of kernels_hdlcrx.hip runs it (HdlcRxSrc::fill: sign words by ballot, NRZI and the descrambler as shifts and XORs on 64-bit
// words in VIRTUAL coordinates, the carried history patched in, the carried decoded bits in front), against the reference's
// bit-serial machines written out here: BinarySlicer (src/binary_slicer.rs:17-19), XorConst(1), NrziDecode (src/nrzi.rs:36-41)
// and Lfsr::next_descramble (src/descrambler.rs:34-39).  No HIP; built by tests/test_hdlcrx_cpu.py with g++:
//   configurations: G3RUH (0x21, 0, 16), a mask with a delay of 64 (len 63), a non-zero seed, every RR_BITS_* combination
//   stream lengths 0, 1, 63, 64, 65 and 4,097, whole and cut into two pushes at every point up to 130
//   behind 8, 63, 64, 65, 200 and 4,101 carried bits, so the symbols start at every kind of place in a word and in a tile
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "hdlcrx_core.hpp"

using namespace rr;
typedef unsigned long long u64;

static int fails = 0;
#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                          \
    } while (0)

struct Cfg {
    bool invert, nrzi, descramble;
    u64 mask, seed;
    unsigned len;
};

// ---- the reference, bit by bit -----------------------------------------------------------------------------------------------------------
struct Serial {
    Cfg c;
    unsigned last = 0;
    u64 shift_reg;
    explicit Serial(const Cfg& cfg) : c(cfg), shift_reg(cfg.seed) {}
    unsigned step(float x) {
        unsigned b = x > 0.0f ? 1u : 0u;
        if (c.invert) b ^= 1u;
        if (c.nrzi) { const unsigned t = last; last = b; b = 1u ^ b ^ t; }
        if (c.descramble) {
            const unsigned ret = (unsigned)(__builtin_popcountll(shift_reg & c.mask) & 1) ^ b;
            shift_reg = (shift_reg >> 1) | ((u64)b << c.len);
            b = ret;
        }
        return b;
    }
};

// ---- the device's steps, thread by thread ----------------------------------------------------------------------------------------------
constexpr long T = 4096, HW = 2, NW = HW + T / 64;
struct Emu {
    Cfg c;
    u64 dmask = 0, st[RX_ST_N] = {0, 0, 0};
    explicit Emu(const Cfg& cfg) : c(cfg) {
        if (c.descramble) { dmask = rx_dmask(c.mask, c.len); st[RX_ST_DHIST] = rx_dhist0(c.seed, c.len); }
    }
    bool rbit(const float* x, long C, long nv, long v) const {
        if (v >= C) return v < nv && (x[v - C] > 0.0f) != c.invert;
        return v == C - 1 && st[RX_ST_RLAST] != 0;
    }
    // one push of n symbols behind the C carried (decoded) bits cin -> the virtual stream's words; the state moves on
    void push(const float* x, long n, const std::vector<uint8_t>& cin, std::vector<u64>& words, std::vector<u64>& prevs) {
        const long C = (long)cin.size(), nv = C + n, ntiles = n ? (nv + T - 1) / T : 0;
        words.assign((size_t)ntiles * (T / 64), 0);
        prevs.assign((size_t)ntiles, 0);
        u64 out[RX_ST_N] = {st[0], st[1], st[2]};
        for (long tile = 0; tile < ntiles; tile++) {
            const long t0 = tile * T;
            u64 s_r[NW] = {0}, s_d[NW] = {0}, s_c[T / 64] = {0}, s_s1 = 0;
            for (long k = 0; k < NW; k++)              // the ballots
                for (int b = 0; b < 64; b++) {
                    const long v = t0 - 64 * HW + 64 * k + b;
                    if (rbit(x, C, nv, v)) s_r[k] |= 1ull << b;
                    if (k >= HW && t0 < C && v < C && (cin[(size_t)v] & 1u)) s_c[k - HW] |= 1ull << b;
                }
            for (long k = 0; k < NW; k++)
                s_d[k] = rx_patch_d(rx_nrzi_word(s_r[k], k ? s_r[k - 1] : 0ull, c.nrzi), t0 - 64 * HW + 64 * k, C, st[RX_ST_DHIST]);
            for (long k = 1; k < NW; k++) {
                const long vb = t0 - 64 * HW + 64 * k;
                const u64 s = rx_descramble_word(s_d[k], s_d[k - 1], dmask);
                if (k >= HW) words[(size_t)(tile * (T / 64) + k - HW)] = rx_final_word(s, t0 < C ? s_c[k - HW] : 0ull, vb, C, nv);
                else s_s1 = rx_final_word(s, 0ull, vb, C, nv);
            }
            if (nv > C && nv - 1 >= t0 && nv - 1 < t0 + T) {
                const long p = nv - 1 - (t0 - 64 * HW);
                out[RX_ST_RLAST] = s_r[p >> 6] >> (p & 63) & 1ull;
                out[RX_ST_DHIST] = rx_win64(s_d, p);
                out[RX_ST_POS] = st[RX_ST_POS] + (u64)(nv - C);
            }
            u64 h = 0;
            for (int lane = 0; lane < 8; lane++) {
                const long v = t0 - 8 + lane;
                if (v >= 0 && (v < C ? (cin[(size_t)v] & 1u) != 0 : (s_s1 >> (v & 63) & 1ull) != 0)) h |= 1ull << lane;
            }
            prevs[(size_t)tile] = h << 56;
        }
        for (int k = 0; k < RX_ST_N; k++) st[k] = out[k];
    }
};

static std::vector<float> draw(std::mt19937& rng, long n) {
    static const float odd[] = {0.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                                -std::numeric_limits<float>::infinity(), 1e-45f, -1e-45f};
    std::vector<float> x((size_t)n);
    for (auto& v : x) {
        const unsigned r = rng();
        v = r % 16 == 0 ? odd[(r >> 8) % 7] : ((r >> 4) & 1 ? 1.0f : -1.0f) * (float)((r >> 8) % 1000 + 1) / 500.0f;
    }
    return x;
}

// the stream x in the pushes `cuts` (their lengths), each behind `carries` carried bits, against the serial machine
static void one(const Cfg& cfg, const std::vector<float>& x, const std::vector<long>& cuts, long carried, std::mt19937& rng, const char* what) {
    Serial ser(cfg);
    Emu emu(cfg);
    long at = 0;
    for (long n : cuts) {
        std::vector<uint8_t> cin((size_t)carried);
        for (auto& b : cin) b = (uint8_t)(rng() & 1u);
        std::vector<u64> words, prevs;
        emu.push(x.data() + at, n, cin, words, prevs);
        const long nv = carried + n;
        for (long v = 0; v < (long)words.size() * 64; v++) {
            const unsigned got = (unsigned)(words[(size_t)(v >> 6)] >> (v & 63) & 1ull);
            unsigned want = 0;
            if (v < carried) want = cin[(size_t)v] & 1u;
            else if (v < nv) want = ser.step(x[(size_t)(at + v - carried)]);
            CHECK(got == want, "%s: carried %ld, push of %ld at %ld: virtual bit %ld is %u, not %u", what, carried, n, at, v, got, want);
            if (fails) return;
            if (v % T == 0 && v) {                 // the 8 bits in front of a tile are the 8 bits of the tile in front
                const u64 top = words[(size_t)((v >> 6) - 1)] & (0xffull << 56);
                CHECK(prevs[(size_t)(v / T)] == top, "%s: the bits in front of tile %ld", what, v / T);
            }
        }
        if (n == 0) CHECK(words.empty(), "%s: an empty push has no tiles", what);
        at += n;
        CHECK(emu.st[RX_ST_POS] == (u64)at, "%s: position %llu after %ld symbols", what, emu.st[RX_ST_POS], at);
    }
}

int main() {
    std::mt19937 rng(20240917);
    std::vector<Cfg> cfgs;
    for (int f = 0; f < 8; f++) cfgs.push_back(Cfg{(f & 1) != 0, (f & 2) != 0, (f & 4) != 0, 0x21, 0, 16});        // every RR_BITS_* combination, G3RUH
    cfgs.push_back(Cfg{false, true, true, 0x8000000000000001ull, 0, 63});                                         // delays 64 and 1
    cfgs.push_back(Cfg{true, true, true, 0x21, 0x1ace5, 16});                                                     // a non-zero seed
    cfgs.push_back(Cfg{false, false, true, 0x5a5a5a5a5a5a5a5aull, 0x7fffffffffffffffull, 62});                    // many delays, a full register
    cfgs.push_back(Cfg{false, true, true, 0x1, 0x1, 0});                                                          // len 0: delay 1 alone
    const long lens[] = {0, 1, 63, 64, 65, 4097}, carries[] = {8, 63, 64, 65, 200, 4101};
    long runs = 0;
    for (const Cfg& c : cfgs)
        for (long n : lens) {
            const std::vector<float> x = draw(rng, n);
            for (long C : carries) {
                one(c, x, {n}, C, rng, "whole");
                runs++;
                for (long cut = 0; cut <= n && cut <= 130; cut++) { one(c, x, {cut, n - cut}, C, rng, "two pushes"); runs++; }
            }
            // and three pushes with an empty one in the middle: the state is kept
            one(c, x, {n / 2, 0, n - n / 2}, 8, rng, "empty push between");
        }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("%ld runs\nhdlcrx core ok\n", runs);
    return 0;
}
