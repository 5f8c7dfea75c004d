// emu_il2p.cpp — rustradio_amd/csrc/il2p_core.hpp under g++, thread by thread as kernels_il2p.hip uses it, against bit-serial code
// written here: the correlator with its slide (src/correlate_access_code.rs:93-118), the chain rule as a walk over positions, the
// bit-serial Lfsr (src/il2p_deframer.rs:107-128), bits_to_bytes and Header::parse.  Prints "il2p core ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "il2p_core.hpp"

using namespace rr;
typedef unsigned long long u64;

static const int SYNC[24] = {1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0};
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// ---- the bit-serial side -----------------------------------------------------------------------------------------------------------
struct SerialRec { long pos; int diffs; unsigned char raw[15]; };
struct Serial {                               // one stream: the correlator's slide, free_from, the open header
    std::vector<int> slide;
    long pos = 0, free_from = 0, open_tag = -1;
    int open_diffs = 0;
    std::vector<int> partial;
    u64 syncs = 0;
    void push(const std::vector<int>& b, unsigned allowed, std::vector<SerialRec>& out) {
        for (int a : b) {
            if (open_tag >= 0) {
                partial.push_back(a);
                if (partial.size() == 120) {
                    SerialRec r{open_tag, open_diffs, {}};
                    u64 sr = 0x1f0;
                    int o[120];
                    for (int k = 0; k < 120; k++) {
                        const int i = partial[k];
                        o[k] = 1 & (i ^ (int)sr);
                        sr = (sr >> 1) ^ (0x108ull * (u64)i);
                    }
                    for (int k = 0; k < 120; k++) r.raw[k / 8] |= (unsigned char)(o[k] << (7 - k % 8));
                    out.push_back(r);
                    open_tag = -1;
                    partial.clear();
                }
            }
            slide.push_back(a);
            if (slide.size() > 24) slide.erase(slide.begin());
            int diffs = 0;
            for (size_t k = 0; k < slide.size(); k++) diffs += slide[k] != SYNC[k];
            if (slide.size() == 24 && (unsigned)diffs <= allowed) {
                syncs++;
                if (pos >= free_from) { open_tag = pos; open_diffs = diffs; free_from = pos + 121; }
            }
            pos++;
        }
    }
};

// ---- the kernels' side: one stream, the three launches with their loops over threads -----------------------------------------------------
struct Emu {
    u64 st[IL2P_ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
    u64 syncs = 0;
    std::vector<u64> all_tags;                // stream positions of every tag, for the match-word checks
    void push(const std::vector<int>& b, unsigned allowed, std::vector<Il2pRec>& out) {
        const long n = (long)b.size();
        if (n == 0) return;                   // k_il2p_scan copies the state
        const long nt = (n + IL2P_T - 1) / IL2P_T;
        std::vector<u64> W(IL2P_CARRY_WORDS + nt * IL2P_TW + 1, 0), mw(nt * IL2P_TW, 0);
        std::vector<unsigned char> maps(nt * IL2P_MAP_PITCH, 0), entry(nt, 0);
        const u64 pos0 = st[IL2P_ST_POS], seen0 = st[IL2P_ST_SEEN];
        const int blocked0 = (int)st[IL2P_ST_BLOCKED];
        const long nv = IL2P_CARRY + n, first = il2p_first_valid(seen0);
        // k_il2p_mark
        for (int k = 0; k < IL2P_CARRY_WORDS; k++) W[k] = st[IL2P_ST_BITS + k];
        for (long i = 0; i < n; i++)
            if (b[i]) W[IL2P_CARRY_WORDS + (i >> 6)] |= 1ull << (i & 63);
        for (long t = 0; t < nt; t++) {
            const long i0 = t * IL2P_T, len = n - i0 < IL2P_T ? n - i0 : IL2P_T;
            u64* m = &mw[t * IL2P_TW];
            for (int tid = 0; tid < IL2P_TW; tid++) {
                const long wi = IL2P_CARRY_WORDS + t * IL2P_TW + tid, vb = IL2P_CARRY + i0 + 64 * tid;
                if (allowed == 0 || allowed >= 24) m[tid] = il2p_match_word(W[wi], W[wi - 1], allowed, vb, first, nv);
                else {
                    u64 ballot = 0;
                    for (int lane = 0; lane < 64; lane++)
                        if ((unsigned)il2p_diffs_at(W[wi], W[wi - 1], lane) <= allowed) ballot |= 1ull << lane;
                    m[tid] = ballot & ~il2p_below(vb, first) & il2p_below(vb, nv);
                    CHECK(m[tid] == il2p_match_word(W[wi], W[wi - 1], allowed, vb, first, nv), "the two forms of the match word");
                }
                syncs += (u64)il2p_popc(m[tid]);
                for (int j = 0; j < 64; j++)
                    if (m[tid] >> j & 1) all_tags.push_back(pos0 + (u64)(i0 + 64 * tid + j));
            }
            for (int e = 0; e < IL2P_STATES; e++) maps[t * IL2P_MAP_PITCH + e] = (unsigned char)il2p_tile_exit(m, len, e);
        }
        // k_il2p_scan: 16 chunks side by side, then the chunks in order
        const int SW = 16;
        const long chunk = (nt + SW - 1) / SW;
        unsigned char comp[SW][IL2P_MAP_PITCH];
        int ent[SW];
        for (int w = 0; w < SW; w++) {
            const long t0 = std::min<long>(w * chunk, nt), t1 = std::min<long>(t0 + chunk, nt);
            for (int e = 0; e < IL2P_STATES; e++) {
                int x = e;
                for (long t = t0; t < t1; t++) x = maps[t * IL2P_MAP_PITCH + x];
                comp[w][e] = (unsigned char)x;
            }
        }
        int e = blocked0;
        for (int w = 0; w < SW; w++) { ent[w] = e; e = comp[w][e]; }
        const int exit_state = e;
        for (int w = 0; w < SW; w++) {
            const long t0 = std::min<long>(w * chunk, nt), t1 = std::min<long>(t0 + chunk, nt);
            int x = ent[w];
            for (long t = t0; t < t1; t++) { entry[t] = (unsigned char)x; x = maps[t * IL2P_MAP_PITCH + x]; }
        }
        // k_il2p_emit
        for (long t = 0; t < nt; t++) {
            const long i0 = t * IL2P_T, len = n - i0 < IL2P_T ? n - i0 : IL2P_T;
            std::vector<long> tags;
            if (t == 0 && blocked0 > 0) tags.push_back((long)blocked0 - IL2P_STATES);
            long p = entry[t];
            for (;;) {
                const long q = il2p_next_tag(&mw[t * IL2P_TW], len, p);
                if (q >= len) break;
                tags.push_back(i0 + q);
                p = q + IL2P_STATES;
            }
            CHECK(tags.size() <= 64, "a lane per tag: %zu", tags.size());
            for (long mine : tags)
                if (mine + IL2P_HEADER_BITS < n) out.push_back(il2p_record(W.data(), IL2P_CARRY + mine, (u64)((long long)pos0 + mine), 0));
        }
        // the state (k_il2p_scan's tail)
        u64 so[IL2P_ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
        so[IL2P_ST_POS] = pos0 + (u64)n;
        so[IL2P_ST_SEEN] = std::min<u64>(seen0 + (u64)n, 24);
        so[IL2P_ST_BLOCKED] = (u64)exit_state;
        for (int k = 0; k < IL2P_CARRY_WORDS; k++) so[IL2P_ST_BITS + k] = il2p_win(W.data(), n + 64 * k);
        std::memcpy(st, so, sizeof st);
    }
};

static std::mt19937_64 rng(20260521);
static std::vector<int> random_bits(long n, int plant_every) {
    std::vector<int> b(n);
    for (auto& x : b) x = (int)(rng() & 1);
    if (plant_every)
        for (long at = (long)(rng() % 40); at + 24 <= n; at += plant_every + (long)(rng() % 7))
            for (int k = 0; k < 24; k++) b[at + k] = SYNC[k] ^ (rng() % 29 == 0);
    return b;
}
static void compare(const std::vector<int>& b, const std::vector<long>& cuts, unsigned allowed, const char* what) {
    Serial s;
    Emu e;
    std::vector<SerialRec> want;
    std::vector<Il2pRec> got;
    long at = 0;
    for (size_t k = 0; k <= cuts.size(); k++) {
        const long end = k < cuts.size() ? cuts[k] : (long)b.size();
        const std::vector<int> part(b.begin() + at, b.begin() + end);
        const size_t w0 = want.size(), g0 = got.size();
        s.push(part, allowed, want);
        e.push(part, allowed, got);
        CHECK(want.size() - w0 == got.size() - g0, "%s: n %zu allowed %u part %zu: %zu headers in this push, want %zu", what, b.size(), allowed,
              k, got.size() - g0, want.size() - w0);
        at = end;
    }
    CHECK(s.syncs == e.syncs, "%s: n %zu allowed %u: %llu tags, want %llu", what, b.size(), allowed, e.syncs, s.syncs);
    CHECK(e.st[IL2P_ST_POS] == (u64)b.size(), "%s: position", what);
    for (size_t i = 0; i < want.size(); i++) {
        CHECK((long)got[i].pos == want[i].pos && got[i].diffs == want[i].diffs, "%s: n %zu allowed %u header %zu: pos %llu diffs %d, want %ld %d",
              what, b.size(), allowed, i, got[i].pos, got[i].diffs, want[i].pos, want[i].diffs);
        CHECK(std::memcmp(got[i].raw, want[i].raw, 15) == 0, "%s: header %zu: raw", what, i);
    }
}

int main() {
    // 1. match words and the whole chain: lengths 0 .. 4,097, whole and cut in two at every point up to 150
    const long lens[] = {0, 1, 23, 24, 63, 64, 65, 4097};
    const unsigned alloweds[] = {0, 1, 3, 24};
    for (unsigned allowed : alloweds)
        for (long n : lens) {
            std::vector<int> b = random_bits(n, 37);
            if (n >= 24) for (int k = 0; k < 24; k++) b[k] = SYNC[k];       // a tag at position 23, the first that can carry one
            compare(b, {}, allowed, "whole");
            for (long cut = 0; cut <= std::min<long>(n, 150); cut++) compare(b, {cut}, allowed, "cut in two");
        }
    // the start-of-stream rule: with every position a match nothing is tagged before position 23
    {
        Emu e;
        std::vector<Il2pRec> got;
        e.push(std::vector<int>(10, 0), 24, got);
        e.push(std::vector<int>(40, 0), 24, got);
        CHECK(e.syncs == 27 && e.all_tags.front() == 23, "start of stream: %llu tags from %llu", e.syncs, e.all_tags.front());
    }
    // several tiles, several pushes, dense and sparse
    for (unsigned allowed : alloweds)
        for (int rep = 0; rep < 3; rep++) {
            const long n = 3 * IL2P_T + 77 + (long)(rng() % 5000);
            const std::vector<int> b = random_bits(n, rep == 0 ? 0 : 150);
            compare(b, {}, allowed, "tiles");
            compare(b, {(long)(rng() % n)}, allowed, "tiles cut");
            std::vector<long> cuts;
            for (long at = 1 + (long)(rng() % 300); at < n; at += 1 + (long)(rng() % 3000)) cuts.push_back(at);
            compare(b, cuts, allowed, "tiles in many pushes");
        }

    // 2. the descramble, the packing and the parse on 1,000 random headers
    for (int rep = 0; rep < 1000; rep++) {
        int in[120], o[120];
        u64 x0 = 0, x1 = 0, sr = 0x1f0;
        for (int k = 0; k < 120; k++) {
            in[k] = (int)(rng() & 1);
            if (in[k]) (k < 64 ? x0 : x1) |= 1ull << (k & 63);
            o[k] = 1 & (in[k] ^ (int)sr);
            sr = (sr >> 1) ^ (0x108ull * (u64)in[k]);
        }
        x1 |= rng() << 56;                                // what stands behind the header in the stream must not matter
        unsigned char want[15] = {0}, raw[15];
        for (int k = 0; k < 120; k++) want[k / 8] |= (unsigned char)(o[k] << (7 - k % 8));
        u64 y0, y1;
        il2p_descramble(x0, x1, &y0, &y1);
        il2p_header_bytes(y0, y1, raw);
        CHECK(std::memcmp(raw, want, 15) == 0, "descramble %d", rep);
        Il2pRec r{};
        il2p_parse(raw, &r);
        const unsigned char* d = want;
        std::string dst, src;
        for (int i = 0; i < 6; i++) { if (d[i] & 63) dst += (char)((d[i] & 63) + 0x20); if (d[6 + i] & 63) src += (char)((d[6 + i] & 63) + 0x20); }
        CHECK(dst == std::string(r.dst, strnlen(r.dst, 7)) && src == std::string(r.src, strnlen(r.src, 7)), "callsigns %d", rep);
        CHECK(r.dst[6] == 0 && r.src[6] == 0, "NUL padded");
        CHECK(r.dst_ssid == d[12] >> 4 && r.src_ssid == (d[12] & 0xf), "ssids");
        CHECK(r.flags == (((d[0] & 0x40) ? 1 : 0) | ((d[0] & 0x80) ? 2 : 0) | ((d[1] & 0x80) ? 4 : 0)), "flags");
        CHECK(r.pid == (((d[1] & 0x40) >> 3) | ((d[2] & 0x40) >> 4) | ((d[3] & 0x40) >> 5) | ((d[4] & 0x40) >> 6)), "pid");
        CHECK(r.control == ((d[5] & 0x40) | ((d[6] & 0x40) >> 1) | ((d[7] & 0x40) >> 2) | ((d[8] & 0x40) >> 3) | ((d[9] & 0x40) >> 4) |
                            ((d[10] & 0x40) >> 5) | ((d[11] & 0x40) >> 6)), "control");
        CHECK(r.payload_size == (((d[2] & 0x80) << 2) | ((d[3] & 0x80) << 1) | (d[4] & 0x80) | ((d[5] & 0x80) >> 1) | ((d[6] & 0x80) >> 2) |
                                 ((d[7] & 0x80) >> 3) | ((d[8] & 0x80) >> 4) | ((d[9] & 0x80) >> 5) | ((d[10] & 0x80) >> 6) | ((d[11] & 0x80) >> 7)), "payload_size");
    }

    // 3. tile maps composed over 1 .. 9 tiles against a serial walk, for every entry state
    for (int kind = 0; kind < 4; kind++)
        for (int ntl = 1; ntl <= 9; ntl++) {
            const long n = (long)(ntl - 1) * IL2P_T + 1 + (long)(rng() % IL2P_T);
            for (int e0 = 0; e0 < IL2P_STATES; e0++) {
                std::vector<u64> m((size_t)ntl * IL2P_TW, 0);
                auto set = [&](long q) { if (q >= 0 && q < n) m[q >> 6] |= 1ull << (q & 63); };
                if (kind == 0) for (long q = (long)(rng() % 300); q < n; q += 1 + (long)(rng() % 400)) set(q);        // sparse
                if (kind == 1) for (long q = 0; q < n; q++) set(q);                                                 // every bit a match
                if (kind == 2) { set(e0 - 1); for (long q = e0 + 500; q < n; q += 121) { set(q); set(q + 120); } }    // at free_from - 1: dropped
                if (kind == 3) { set(e0); for (long q = e0 + 121; q < n; q += 121) set(q); }                        // at free_from: accepted
                // the serial walk over positions
                long free_from = e0;
                for (long q = 0; q < n; q++)
                    if ((m[q >> 6] >> (q & 63) & 1) && q >= free_from) free_from = q + 121;
                const int want = (int)std::max<long>(free_from - n, 0);
                unsigned char acc[IL2P_MAP_PITCH], one[IL2P_MAP_PITCH], nxt[IL2P_MAP_PITCH];
                for (int t = 0; t < ntl; t++) {
                    const long len = std::min<long>(n - (long)t * IL2P_T, IL2P_T);
                    il2p_tile_map(&m[(size_t)t * IL2P_TW], len, one);
                    if (t == 0) std::memcpy(acc, one, sizeof acc);
                    else { il2p_map_then(acc, one, nxt); std::memcpy(acc, nxt, sizeof acc); }
                }
                CHECK(acc[e0] == want, "maps: kind %d tiles %d entry %d: exit %d, want %d", kind, ntl, e0, acc[e0], want);
            }
        }
    std::printf("il2p core ok\n");
    return 0;
}
