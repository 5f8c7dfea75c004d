// emu_hdlc.cpp — the arithmetic of rustradio_amd/csrc/hdlc_core.hpp on the CPU, run thread by thread the way kernels_hdlc.hip
// runs it (word per lane, gap per thread, 64 lanes per frame), against the reference's sequential machine written out here
// (src/hdlc_deframer.rs:123-232, find_right_crc :41-71, calc_crc :309-315).  No HIP; built by tests/test_hdlc_dev_cpu.py with g++:
//   1. predicates, gap maps, the resolved chain and the frames: every bit string of up to 20 bits behind every entry state (S, U3,
//      U: one, two, three flags sharing their zeros), followed by a frame that shows the state it left; strings of up to 10
//      bits also cut into two pushes at every point
//   2. the composition of maps, associative over every map the gaps can produce and everything they compose to
//   3. CRC chunks combined by x^(8 len) against the table CRC
//   4. the syndrome search against brute-force find_right_crc for bodies of 1, 2, 24, 1500 and 4,200 bytes, and a constructed
//      two-hit case at 4,200
//   5. the carry bound: reached by the stuffed all-ones frame, never exceeded, for max_size 0, 1, 3, 1500
//   6. drawn streams cut into random pushes, every flag combination; long frames (up to 1,497 bytes, all-ones ones among them)
//      with and without a flipped bit
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "hdlc_core.hpp"

using namespace rr;
typedef unsigned long long u64;

static int fails = 0;
#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                          \
    } while (0)

// ---- the reference, sequentially ---------------------------------------------------------------------------------------------------------
static unsigned g_table[256];
static void make_table() {
    for (unsigned b = 0; b < 256; b++) {
        unsigned v = b;
        for (int i = 0; i < 8; i++) v = (v >> 1) ^ ((v & 1u) ? 0x8408u : 0u);
        g_table[b] = v;
    }
}
static unsigned table_crc(const uint8_t* d, size_t n) {
    unsigned fcs = 0xffffu;
    for (size_t i = 0; i < n; i++) fcs = (fcs >> 8) ^ g_table[(fcs ^ d[i]) & 0xffu];
    return fcs ^ 0xffffu;
}
// -> crc; *fixed; data repaired in place when a data bit was found
static unsigned find_right_crc(std::vector<uint8_t>& data, unsigned got, bool fix_bits, bool* fixed, bool* newdata) {
    *fixed = *newdata = false;
    const unsigned crc = table_crc(data.data(), data.size());
    if (got == crc || !fix_bits) return crc;
    for (size_t byte = 0; byte < data.size(); byte++)
        for (int bit = 0; bit < 8; bit++) {
            data[byte] ^= (uint8_t)(1u << bit);
            const unsigned c = table_crc(data.data(), data.size());
            if (c == got) { *fixed = *newdata = true; return c; }
            data[byte] ^= (uint8_t)(1u << bit);
        }
    for (int k = 0; k < 16; k++)
        if ((got ^ (1u << k)) == crc) { *fixed = true; return got ^ (1u << k); }
    return crc;
}
struct Frame {
    u64 pos;
    std::vector<uint8_t> data;
    bool fixed;
    bool operator==(const Frame& o) const { return pos == o.pos && data == o.data && fixed == o.fixed; }
};
struct Seq {
    size_t mn, mx;
    bool keep, fix;
    int state = 0;                              // 0 Unsynced, 1 Synced, 2 FinalCheck
    unsigned reg = 0xff, ones = 0;
    std::vector<uint8_t> bits;
    u64 stats[3] = {0, 0, 0}, pos = 0;
    Seq(size_t a, size_t b, bool k, bool f) : mn(a), mx(b), keep(k), fix(f) {}
    void unsync() { state = 0; reg = 0xff; bits.clear(); }
    void sync() { state = 1; ones = 0; bits.clear(); }
    void step(unsigned bit, std::vector<Frame>& out) {
        if (state == 0) {
            const unsigned n = (reg >> 1) | (bit << 7);
            if (n == 0x7e) sync(); else reg = n;
        } else if (state == 1) {
            if (bits.size() > mx * 8) { unsync(); return; }
            if (bit) {
                bits.push_back(1);
                if (ones == 5) state = 2; else ones++;
            } else if (ones == 5) {
                ones = 0;
            } else {
                bits.push_back(0);
                ones = 0;
            }
        } else {
            if (bit || bits.size() < 7) { unsync(); return; }
            std::vector<uint8_t> b(bits.begin(), bits.end() - 7);
            sync();
            if (b.size() % 8 || b.size() / 8 < mn) return;
            std::vector<uint8_t> data(b.size() / 8, 0);
            for (size_t i = 0; i < b.size(); i++) data[i / 8] |= (uint8_t)(b[i] << (i % 8));
            if (keep) { stats[0]++; out.push_back(Frame{pos, data, false}); return; }
            if (data.size() < 2) return;
            const unsigned got = data[data.size() - 2] | data[data.size() - 1] << 8;
            data.resize(data.size() - 2);
            bool fixed, nd;
            const unsigned crc = find_right_crc(data, got, fix, &fixed, &nd);
            if (fixed) stats[2]++;
            if (crc != got) { stats[1]++; return; }
            stats[0]++;
            out.push_back(Frame{pos, data, fixed});
        }
    }
    void run(const uint8_t* b, size_t n, std::vector<Frame>& out) {
        for (size_t i = 0; i < n; i++, pos++) step(b[i] & 1u, out);
    }
};

// ---- the device's steps, thread by thread -------------------------------------------------------------------------------------------------
struct Emu {
    static constexpr long GB = 4;               // gaps of one block of the map scan (the kernels' HDLC_GB, small to cross many seams)
    size_t mn, mx;
    bool keep, fix;
    std::vector<uint8_t> cbits;
    int state = HDLC_U;
    u64 stats[3] = {0, 0, 0}, w0 = 0;
    std::vector<u64> raw, fl, ab, sf;
    std::vector<long> ends;
    std::vector<hdlc_map> gmap, pmap, bmap;
    std::vector<int> bstate;
    Emu(size_t a, size_t b, bool k, bool f) : mn(a), mx(b), keep(k), fix(f), cbits(HDLC_HALO, 1) {}
    void push(const uint8_t* bits, size_t n, std::vector<Frame>& out) {
        if (!n) return;
        const long C = (long)cbits.size(), nv = C + (long)n, nw = (nv + 63) / 64;
        raw.assign(nw + 1, 0); fl.assign(nw + 1, 0); ab.assign(nw + 1, 0); sf.assign(nw + 1, 0);
        for (long v = 0; v < nv; v++)
            if ((v < C ? cbits[v] : bits[v - C]) & 1u) raw[v >> 6] |= 1ull << (v & 63);
        ends.clear();
        for (long w = 0; w < nw; w++) {         // k_hdlc_mark's lane
            HdlcMarks m = hdlc_marks(raw[w], w ? raw[w - 1] : 0ull);
            const long v0 = 64 * w;
            u64 valid = nv - v0 >= 64 ? ~0ull : (1ull << (nv - v0)) - 1ull;
            if (v0 == 0) valid &= ~0ull << HDLC_HALO;
            fl[w] = m.flag & valid; ab[w] = m.abort & valid; sf[w] = m.stuffed & valid;
            for (u64 f = fl[w]; f; f &= f - 1) ends.push_back(v0 + hdlc_ctz(f));
        }
        const long E = (long)ends.size(), nb = (E + GB - 1) / GB;
        gmap.assign(E, 0); pmap.assign(E, 0); bmap.assign(nb, 0); bstate.assign(nb, 0);
        for (long b = 0; b < nb; b++) {         // k_hdlc_gap's block
            hdlc_map run = HDLC_MAP_ID;
            for (long j = b * GB; j < E && j < (b + 1) * GB; j++) {
                gmap[j] = hdlc_gap_scan(ab.data(), sf.data(), j ? ends[j - 1] : HDLC_HALO - 1, ends[j], mx).map;
                pmap[j] = run;
                run = hdlc_map_then(run, gmap[j] & HDLC_MAP_MASK);
            }
            bmap[b] = run;
        }
        hdlc_map all = HDLC_MAP_ID;             // k_hdlc_resolve
        for (long b = 0; b < nb; b++) { bstate[b] = hdlc_map_at(all, state); all = hdlc_map_then(all, bmap[b]); }
        const int fin = hdlc_map_at(all, state);
        for (long j = 0; j < E; j++) emit(j, C, out);
        const HdlcCarry c = hdlc_carry_plan(E ? ends[E - 1] : HDLC_HALO - 1, fin, nv, mx);
        std::vector<uint8_t> next(c.count);
        for (long i = 0; i < c.count; i++) next[i] = (uint8_t)(raw[(c.from + i) >> 6] >> ((c.from + i) & 63) & 1ull);
        cbits.swap(next);
        state = c.state;
        w0 += n;
    }
    void emit(long j, long C, std::vector<Frame>& out) {        // k_hdlc_emit's wave
        if (!(gmap[j] & HDLC_EMITS) || hdlc_map_at(pmap[j], bstate[j / GB]) != HDLC_S) return;
        const long s = j ? ends[j - 1] : HDLC_HALO - 1, f = ends[j];
        u64 kept = 0;
        for (long p = s + 1; p < f; p++) kept += 1 - (sf[p >> 6] >> (p & 63) & 1ull);
        const long nbytes = hdlc_frame_bytes(kept, mn);
        if (nbytes < 0 || (!keep && nbytes < 2)) return;
        const long blen = keep ? nbytes : nbytes - 2, ch = (nbytes + 63) / 64;
        std::vector<uint8_t> data(blen, 0);
        unsigned diff = 0;
        long c0s[64], c1s[64];
        // the gap's words in 64 segments, one per lane: the kept bits in front of each
        const long wf = (s + 1) >> 6, wl = (f - 1) >> 6, seg = (wl - wf + 64) / 64;
        u64 before[64], run = 0;
        for (int lane = 0; lane < 64; lane++) {
            before[lane] = run;
            for (long w = wf + lane * seg; w < wf + (lane + 1) * seg && w <= wl; w++)
                for (long p = std::max(s + 1, w << 6); p < std::min(f, (w + 1) << 6); p++) run += 1 - (sf[w] >> (p & 63) & 1ull);
        }
        CHECK(run == kept, "the segments hold the gap's kept bits");
        for (int lane = 0; lane < 64; lane++) {
            const long k0 = lane * ch < nbytes ? lane * ch : nbytes, k1 = k0 + ch < nbytes ? k0 + ch : nbytes;
            unsigned fcs = 0xffffu, got = 0;
            const int sj = hdlc_seg_find(8 * (u64)k0, [&](int j) { return before[j]; });
            if (k0 < k1) {
                const long p = hdlc_select(sf.data(), hdlc_seg_from(s, wf, seg, sj), f, 8 * (u64)k0 - before[sj]);
                CHECK(p >= 0 && p == hdlc_select(sf.data(), s, f, 8 * (u64)k0), "the search from the segment finds the search from the flag end");
                HdlcCursor c = hdlc_cursor(raw.data(), sf.data(), p < 0 ? s + 1 : p);
                for (long k = k0; k < k1 && p >= 0; k++) {
                    const unsigned byte = hdlc_take_byte(raw.data(), sf.data(), c);
                    if (k < blen) { data[k] = (uint8_t)byte; fcs = crc16_byte(fcs, byte); }
                    else got |= byte << (8 * (unsigned)(k - blen));
                }
                CHECK(c.p <= f - 7, "bytes ran into the closing flag: p %ld f %ld", c.p, f);
            }
            c0s[lane] = k0 < blen ? k0 : blen; c1s[lane] = k1 < blen ? k1 : blen;
            diff ^= (c0s[lane] < c1s[lane] ? hdlc_crc_part(fcs, (u64)(blen - c1s[lane])) : 0u) ^ got;
        }
        const u64 pos = w0 + (u64)f - (u64)C;
        if (keep || diff == 0) { stats[0]++; out.push_back(Frame{pos, data, false}); return; }
        if (!fix) { stats[1]++; return; }
        long hit = -1;
        for (int lane = 0; lane < 64; lane++) {
            const long h = hdlc_syn_search(diff, 8 * (u64)blen, 8 * (u64)c0s[lane], 8 * (u64)c1s[lane]);
            if (h >= 0 && (hit < 0 || h < hit)) hit = h;
        }
        if (hit >= 0) {
            data[hit / 8] ^= (uint8_t)(1u << (hit & 7));
            stats[0]++; stats[2]++;
            out.push_back(Frame{pos, data, true});
        } else {
            if (hdlc_popc(diff) == 1) stats[2]++;
            stats[1]++;
        }
    }
};

static const uint8_t FLAG[8] = {0, 1, 1, 1, 1, 1, 1, 0};
static void add_flag(std::vector<uint8_t>& v) { v.insert(v.end(), FLAG, FLAG + 8); }
static void add_stuffed(std::vector<uint8_t>& v, const std::vector<uint8_t>& bytes) {
    int run = 0;
    for (uint8_t x : bytes)
        for (int k = 0; k < 8; k++) {
            const uint8_t b = x >> k & 1;
            v.push_back(b);
            run = b ? run + 1 : 0;
            if (run == 5) { v.push_back(0); run = 0; }
        }
}
static bool same(const Seq& a, const Emu& b, const std::vector<Frame>& fa, const std::vector<Frame>& fb) {
    return fa == fb && a.stats[0] == b.stats[0] && a.stats[1] == b.stats[1] && a.stats[2] == b.stats[2];
}

static void test_exhaustive() {
    long cases = 0;
    std::vector<uint8_t> s;
    std::vector<Frame> fa, fb;
    const size_t cfgs[3][2] = {{0, 3}, {0, 1}, {1, 0}};
    for (int cfg = 0; cfg < 3; cfg++) {
        const int maxlen = cfg == 0 ? 20 : 12;
        for (int shared = 1; shared <= 3; shared++)             // the entry state: S, U3, U
            for (int n = 0; n <= maxlen; n++)
                for (unsigned x = 0; x < (1u << n); x++) {
                    s.clear();
                    for (int k = 0; k < shared; k++) s.insert(s.end(), FLAG, FLAG + 7);
                    s.push_back(0);
                    for (int i = 0; i < n; i++) s.push_back(x >> i & 1);
                    add_flag(s);
                    add_stuffed(s, {0x15});
                    add_flag(s);
                    const int ncuts = n <= 10 ? (int)s.size() : 1;
                    fa.clear();
                    Seq q(cfgs[cfg][0], cfgs[cfg][1], true, false);
                    q.run(s.data(), s.size(), fa);
                    for (int cut = 0; cut < ncuts; cut++) {
                        fb.clear();
                        Emu e(cfgs[cfg][0], cfgs[cfg][1], true, false);
                        e.push(s.data(), cut, fb);
                        e.push(s.data() + cut, s.size() - cut, fb);
                        CHECK(same(q, e, fa, fb), "cfg %d shared %d n %d x %x cut %d: %zu vs %zu frames", cfg, shared, n, x, cut, fa.size(),
                              fb.size());
                        cases++;
                    }
                }
    }
    std::printf("exhaustive: %ld cases\n", cases);
}

static void test_maps() {
    std::set<hdlc_map> maps;
    for (int share = 0; share < 2; share++)
        for (int reset = 0; reset < 2; reset++)
            for (int hides = 0; hides < 2; hides++) maps.insert(hdlc_gap_map(share, reset, hides) & HDLC_MAP_MASK);
    maps.insert(HDLC_MAP_ID);
    for (bool grew = true; grew;) {             // ... and everything they compose to
        grew = false;
        std::set<hdlc_map> add;
        for (hdlc_map a : maps)
            for (hdlc_map b : maps) add.insert(hdlc_map_then(a, b));
        for (hdlc_map m : add) grew |= maps.insert(m).second;
    }
    for (hdlc_map a : maps)
        for (hdlc_map b : maps)
            for (hdlc_map c : maps) {
                CHECK(hdlc_map_then(hdlc_map_then(a, b), c) == hdlc_map_then(a, hdlc_map_then(b, c)), "not associative: %x %x %x", a, b, c);
                for (int st = 0; st < 3; st++)
                    CHECK(hdlc_map_at(hdlc_map_then(a, b), st) == hdlc_map_at(b, hdlc_map_at(a, st)), "then is not b after a");
            }
    for (hdlc_map a : maps) CHECK(hdlc_map_then(a, HDLC_MAP_ID) == a && hdlc_map_then(HDLC_MAP_ID, a) == a, "identity");
    std::printf("maps: %zu in the closure\n", maps.size());
}

static void test_crc(std::mt19937& rng) {
    for (int it = 0; it < 400; it++) {
        const size_t n = it < 70 ? (size_t)it : rng() % 5000;
        std::vector<uint8_t> d(n);
        for (auto& x : d) x = (uint8_t)rng();
        const size_t ch = (n + 63) / 64;
        unsigned crc = 0;
        for (size_t lane = 0; lane < 64; lane++) {
            const size_t k0 = std::min(lane * ch, n), k1 = std::min(k0 + ch, n);
            unsigned fcs = 0xffffu;
            for (size_t k = k0; k < k1; k++) fcs = crc16_byte(fcs, d[k]);
            if (k0 < k1) crc ^= hdlc_crc_part(fcs, n - k1);
        }
        CHECK(crc == table_crc(d.data(), n), "crc of %zu bytes", n);
    }
    const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    CHECK(table_crc(check, 9) == 0x906e, "check value");
}

// the search as k_hdlc_emit runs it over a body and a received CRC -> what find_right_crc does to a copy
static void one_syndrome(const std::vector<uint8_t>& body, unsigned got, const char* what) {
    std::vector<uint8_t> want = body;
    bool fixed, nd;
    const unsigned crc = find_right_crc(want, got, true, &fixed, &nd);
    const size_t n = body.size(), ch = (n + 63) / 64;
    const unsigned diff = table_crc(body.data(), n) ^ got;
    long hit = -1;
    for (size_t lane = 0; lane < 64 && diff; lane++) {
        const size_t k0 = std::min(lane * ch, n), k1 = std::min(k0 + ch, n);
        const long h = hdlc_syn_search(diff, 8 * n, 8 * k0, 8 * k1);
        if (h >= 0 && (hit < 0 || h < hit)) hit = h;
    }
    std::vector<uint8_t> mine = body;
    if (hit >= 0) mine[hit / 8] ^= (uint8_t)(1u << (hit & 7));
    CHECK((hit >= 0) == nd && mine == want, "%s: %zu bytes, hit %ld, reference %s", what, n, hit, nd ? "repaired" : "did not repair");
    const bool crc_only = hit < 0 && diff && hdlc_popc(diff) == 1;
    CHECK((diff == 0 || hit >= 0) == (crc == got), "%s: delivered or not", what);
    CHECK((hit >= 0 || crc_only) == fixed, "%s: bitfixed", what);
}
static void test_syndrome(std::mt19937& rng) {
    const size_t sizes[5] = {1, 2, 24, 1500, 4200};
    for (size_t n : sizes) {
        const int reps = n <= 24 ? 200 : n == 1500 ? 6 : 3;
        for (int it = 0; it < reps; it++) {
            std::vector<uint8_t> body(n);
            for (auto& x : body) x = (uint8_t)rng();
            const unsigned good = table_crc(body.data(), n);
            std::vector<uint8_t> broken = body;
            const size_t h = it == 0 ? 0 : it == 1 ? 8 * n - 1 : rng() % (8 * n);
            broken[h / 8] ^= (uint8_t)(1u << (h & 7));
            one_syndrome(broken, good, "one data bit");
            one_syndrome(body, good ^ (1u << (rng() % 16)), "one crc bit");
            if (n <= 24) {
                one_syndrome(body, good, "good");
                one_syndrome(body, (unsigned)rng() & 0xffffu, "random crc");
            }
        }
    }
    // two hits: the syndromes repeat every 32767 bits, so a flip 32767 bits behind bit h looks like a flip of bit h
    std::vector<uint8_t> body(4200);
    for (auto& x : body) x = (uint8_t)rng();
    const unsigned good = table_crc(body.data(), body.size());
    const size_t h = 300, far = h + 32767;
    CHECK(far < 8 * body.size(), "the far bit lies inside the body");
    CHECK(hdlc_syn(8 * body.size() - h) == hdlc_syn(8 * body.size() - far), "the period of the polynomial is 32767");
    std::vector<uint8_t> broken = body;
    broken[far / 8] ^= (uint8_t)(1u << (far & 7));
    CHECK(hdlc_syn_search(table_crc(broken.data(), broken.size()) ^ good, 8 * body.size(), 0, 8 * body.size()) == (long)h, "the lowest of two hits");
    one_syndrome(broken, good, "two hits");
}

static void test_carry_bound(std::mt19937& rng) {
    const size_t sizes[4] = {0, 1, 3, 1500};
    for (size_t mx : sizes) {
        const u64 R = hdlc_reset_bits(mx);
        // all ones, stuffed: the machine gives up on the bit behind R raw bits, not sooner
        std::vector<uint8_t> s;
        add_flag(s);
        add_stuffed(s, std::vector<uint8_t>(mx + 2, 0xff));
        Seq q(0, mx, true, false);
        std::vector<Frame> fr;
        long reset_at = -1;
        for (size_t i = 0; i < s.size() && reset_at < 0; i++) {
            const int before = q.state;
            q.step(s[i], fr);
            if (i >= 8 && before == 1 && q.state == 0) reset_at = (long)i - 7;          // raw bits behind the flag end, this one included
        }
        CHECK(reset_at == (long)R + 1, "max_size %zu: all ones reset at raw bit %ld, bound %llu + 1", mx, reset_at, R);
        // whatever the gap holds it has reset by then
        for (int it = 0; it < 300; it++) {
            std::vector<uint8_t> t;
            add_flag(t);
            const int p1 = 50 + (int)(rng() % 50);
            for (u64 i = 0; i < R + 1; i++) t.push_back((int)(rng() % 100) < p1);
            Seq r(0, mx, true, false);
            r.run(t.data(), t.size(), fr);
            CHECK(r.state != 1 || r.bits.size() <= 8 * mx, "max_size %zu: still collecting %zu bits behind the bound", mx, r.bits.size());
        }
        // the emulated handle carries exactly the bound behind such a gap, and 8 bits one bit later
        Emu e(0, mx, true, false);
        std::vector<uint8_t> g;
        add_flag(g);
        add_stuffed(g, std::vector<uint8_t>(mx + 2, 0xff));
        g.resize(8 + hdlc_reach(mx));
        if (mx == 0) for (size_t i = 8; i < g.size(); i++) g[i] = 0;                   // (no room for seven ones: keep the gap free of aborts)
        e.push(g.data(), g.size(), fr);
        const size_t bound = HDLC_HALO + (size_t)hdlc_reach(mx);
        CHECK(e.cbits.size() == bound || e.state == HDLC_U, "max_size %zu: carried %zu, bound %zu", mx, e.cbits.size(), bound);
        if (mx == 1500) CHECK(e.cbits.size() == bound, "max_size 1500: the all-ones gap reaches the bound (carried %zu of %zu)", e.cbits.size(), bound);
        const uint8_t one = 1;
        e.push(&one, 1, fr);
        CHECK(e.cbits.size() == (size_t)HDLC_HALO && e.state == HDLC_U, "max_size %zu: one bit further the gap is cut down", mx);
    }
}

static void draw(std::mt19937& rng, size_t nbits, std::vector<uint8_t>& out) {
    out.clear();
    while (out.size() < nbits) {
        const int kind = rng() % 7, m = 1 + rng() % 39;
        if (kind == 0) for (int i = 0; i < m; i++) out.push_back(rng() & 1);
        else if (kind == 1) for (int i = 0; i < m; i++) out.push_back(rng() % 100 < 85);
        else if (kind == 2) for (int i = 0, k = 1 + rng() % 3; i < k; i++) add_flag(out);
        else if (kind == 3) { for (int i = 0, k = 1 + rng() % 4; i < k; i++) out.insert(out.end(), FLAG, FLAG + 7); out.push_back(0); }
        else if (kind == 4) { for (int i = 0, k = 5 + rng() % 4; i < k; i++) out.push_back(1); out.push_back(0); }
        else {
            std::vector<uint8_t> p(rng() % 6);
            for (auto& x : p) x = (uint8_t)rng();
            if (rng() & 1) { const unsigned c = table_crc(p.data(), p.size()); p.push_back(c & 0xff); p.push_back(c >> 8); }
            const size_t at = out.size();
            add_flag(out);
            add_stuffed(out, p);
            if (rng() & 1) add_flag(out);
            if (rng() % 10 < 3 && out.size() - at > 16) out[at + 8 + rng() % (out.size() - at - 16)] ^= 1;
        }
    }
    out.resize(nbits);
}
static void test_streams(std::mt19937& rng) {
    size_t frames = 0, fixes = 0, carried_max = 0;
    std::vector<uint8_t> s;
    std::vector<Frame> fa, fb;
    for (int it = 0; it < 3000; it++) {
        const size_t mn = rng() % 4, mx = rng() % 11;
        const bool keep = rng() & 1, fix = rng() & 1;
        draw(rng, 1 + rng() % 1500, s);
        Seq q(mn, mx, keep, fix);
        Emu e(mn, mx, keep, fix);
        fa.clear(); fb.clear();
        q.run(s.data(), s.size(), fa);
        const size_t win = it % 3 == 0 ? 1 + rng() % 9 : 1 + rng() % 300;
        for (size_t at = 0; at < s.size();) {
            const size_t n = std::min(s.size() - at, 1 + rng() % win);
            e.push(s.data() + at, n, fb);
            at += n;
            carried_max = std::max(carried_max, e.cbits.size());
            CHECK(e.cbits.size() <= HDLC_HALO + hdlc_reach(mx), "carried %zu bits beyond the bound of max_size %zu", e.cbits.size(), mx);
        }
        CHECK(same(q, e, fa, fb), "stream %d (%zu, %zu, %d, %d): %zu vs %zu frames", it, mn, mx, keep, fix, fa.size(), fb.size());
        frames += fa.size();
        fixes += q.stats[2];
    }
    CHECK(frames > 2000 && fixes > 50, "the drawn streams hold frames (%zu) and repairs (%zu)", frames, fixes);
    std::printf("streams: %zu frames, %zu repairs, at most %zu bits carried\n", frames, fixes, carried_max);
}

// long frames: the 64 lanes take many bytes each, and the gap's words many segments
static void test_long_frames(std::mt19937& rng) {
    std::vector<uint8_t> s;
    std::vector<Frame> fa, fb;
    size_t repaired = 0;
    for (int it = 0; it < 16; it++) {
        s.clear();
        for (int k = 0; k < 2; k++) {
            std::vector<uint8_t> p(it == 0 ? 1497 : 60 + rng() % 1400);
            for (auto& x : p) x = (uint8_t)(it % 3 == 1 ? 0xff : rng());
            const unsigned c = table_crc(p.data(), p.size());
            p.push_back(c & 0xff); p.push_back(c >> 8);
            if (it % 2 && k == 0) p[rng() % 8] ^= (uint8_t)(1u << (rng() % 8));       // (low in the frame: the brute force finds it soon)
            for (unsigned z = rng() % 70; z; z--) s.push_back(0);
            add_flag(s);
            add_stuffed(s, p);
            add_flag(s);
        }
        Seq q(10, 1500, false, true);
        Emu e(10, 1500, false, true);
        fa.clear(); fb.clear();
        q.run(s.data(), s.size(), fa);
        for (size_t at = 0; at < s.size();) {
            const size_t n = std::min(s.size() - at, (size_t)(1 + rng() % 9000));
            e.push(s.data() + at, n, fb);
            at += n;
        }
        CHECK(same(q, e, fa, fb) && fa.size() == 2, "long frames %d: %zu vs %zu frames", it, fa.size(), fb.size());
        repaired += q.stats[2];
    }
    CHECK(repaired == 8, "every second stream holds one repair (%zu)", repaired);
}

int main() {
    make_table();
    std::mt19937 rng(12345);
    test_maps();
    test_crc(rng);
    test_syndrome(rng);
    test_carry_bound(rng);
    test_streams(rng);
    test_long_frames(rng);
    test_exhaustive();
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("hdlc core ok\n");
    return 0;
}
