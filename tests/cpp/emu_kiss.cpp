// emu_kiss.cpp — rustradio_amd/csrc/kiss_core.hpp run thread by thread and tile by tile on the CPU, in the launch order of
// kernels_kiss.hip (k_kiss_sum, k_kiss_scan, k_kiss_pass<1>, k_kiss_scan2, k_kiss_pass<2>, k_kiss_pass<3>), with the state carried
// from push to push as the device carries it.  tests/test_kiss_cpu.py feeds it streams on stdin and compares what it prints with
// tests/kiss_model.py:
//   in:   "max_len tile npushes", then per push "len hex" ("-" for no bytes)
//   out:  "P push pos port in_bytes hex" per packet, "S frames delivered nondata bad_escape overlong" behind every push
// The tile is the emulation's own (a multiple of the 16 bytes of a thread), so that a few hundred bytes cross many tiles.
// With the argument "encode": the encoder's per-byte functions over one hex line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "kiss_core.hpp"

using namespace rr;

static std::vector<unsigned char> unhex(const std::string& h) {
    std::vector<unsigned char> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((unsigned char)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

struct State {
    unsigned long long stats[5] = {0, 0, 0, 0, 0};
    int code = KISS_UNSYNC;
    std::vector<unsigned char> carry;
};
struct Rec {
    long pos;
    unsigned start, len, in_bytes, port;
};

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "encode") == 0) {
        std::string h;
        std::cin >> h;
        for (unsigned char b : unhex(h)) std::printf("%u ", kiss_escapes(b));
        std::printf("ports");
        for (unsigned long long p : {0ull, 1ull, 12ull, 15ull, 16ull, 99ull}) std::printf(" %u", kiss_port_byte(p));
        std::printf("\n");
        return 0;
    }
    long max_len, T, npushes;
    if (!(std::cin >> max_len >> T >> npushes) || T % KISS_LANE) return 2;
    State st;
    long w0 = 0;
    for (long push = 0; push < npushes; push++) {
        long n;
        std::string h;
        std::cin >> n >> h;
        const std::vector<unsigned char> win = unhex(h);
        if ((long)win.size() != n) return 2;
        if (n == 0) {                             // a push of nothing leaves every state alone
            std::printf("S %llu %llu %llu %llu %llu\n", st.stats[0], st.stats[1], st.stats[2], st.stats[3], st.stats[4]);
            continue;
        }
        std::vector<unsigned char> V = st.carry;
        const long c = (long)V.size();
        V.insert(V.end(), win.begin(), win.end());
        const long len = (long)V.size(), ntiles = (len + T - 1) / T, lanes = T / KISS_LANE;
        auto at = [&](long v, int k, bool* has_next) {     // kiss_byte of byte k of the thread that begins at v
            const long i = v + k;
            *has_next = i + 1 < len;
            return kiss_byte((int)i, V[i], *has_next ? V[i + 1] : 0u, *has_next);
        };
        auto lane_sum = [&](long v0) {
            KissSum s = kiss_none();
            bool hn;
            for (int k = 0; k < KISS_LANE && v0 + k < len; k++) s = kiss_combine(s, at(v0, k, &hn));
            return s;
        };
        // k_kiss_sum
        std::vector<KissSum> sums(ntiles), tin(ntiles);
        for (long t = 0; t < ntiles; t++) {
            KissSum s = kiss_none();
            for (long l = 0; l < lanes; l++) s = kiss_combine(s, lane_sum(t * T + l * KISS_LANE));
            sums[t] = s;
        }
        // k_kiss_scan
        KissSum root = kiss_seed(st.code);
        for (long t = 0; t < ntiles; t++) { tin[t] = root; root = kiss_combine(root, sums[t]); }
        // every FEND of a thread: f(run, e, gap)
        auto fends = [&](long v0, KissSum run, auto&& f) {
            bool hn;
            for (int k = 0; k < KISS_LANE && v0 + k < len; k++) {
                if (V[v0 + k] == KISS_FEND) {
                    const long glen = kiss_gap_len(run, (int)(v0 + k));
                    const unsigned port = glen >= 1 && glen <= max_len ? V[run.last + 1] : 0u;
                    f(run, v0 + k, kiss_close(run, glen, (unsigned)max_len, port));
                }
                run = kiss_combine(run, at(v0, k, &hn));
            }
        };
        // k_kiss_pass<1>
        std::vector<unsigned> tsum(5 * ntiles, 0u), toff(2 * ntiles, 0u);
        for (long t = 0; t < ntiles; t++) {
            KissSum ex = tin[t];
            for (long l = 0; l < lanes; l++) {
                fends(t * T + l * KISS_LANE, ex, [&](const KissSum&, long, const KissGap& g) {
                    if (g.kind == KISS_G_DELIVERED) { tsum[5 * t] += 1; tsum[5 * t + 1] += g.len; }
                    else if (g.kind != KISS_G_NOTHING) tsum[5 * t + g.kind] += 1;
                });
                ex = kiss_combine(ex, lane_sum(t * T + l * KISS_LANE));
            }
        }
        // k_kiss_scan2
        unsigned tot[5] = {0, 0, 0, 0, 0};
        for (long t = 0; t < ntiles; t++) {
            toff[2 * t] = tot[0]; toff[2 * t + 1] = tot[1];
            for (int q = 0; q < 5; q++) tot[q] += tsum[5 * t + q];
        }
        State next = st;
        next.stats[0] += tot[0] + tot[2] + tot[3]; next.stats[1] += tot[0]; next.stats[2] += tot[2]; next.stats[3] += tot[3]; next.stats[4] += tot[4];
        unsigned ncarry;
        kiss_next(root, len, (unsigned)max_len, &next.code, &ncarry);
        // k_kiss_pass<2>
        const unsigned NOBASE = 0xffffffffu;
        std::vector<Rec> recs(tot[0]);
        std::vector<unsigned> obase(ntiles + 1, NOBASE);
        auto slot = [&](int last) { return last < 0 ? 0l : (long)(last / T) + 1; };
        for (long t = 0; t < ntiles; t++) {
            KissSum ex = tin[t];
            unsigned pk = toff[2 * t], by = toff[2 * t + 1];
            for (long l = 0; l < lanes; l++) {
                fends(t * T + l * KISS_LANE, ex, [&](const KissSum& run, long e, const KissGap& g) {
                    if (g.kind != KISS_G_DELIVERED) return;
                    recs[pk] = Rec{w0 + (e - c), by, g.len, g.in_bytes, g.port};
                    if (slot(run.last) != t + 1) obase[slot(run.last)] = by;
                    pk += 1; by += g.len;
                });
                ex = kiss_combine(ex, lane_sum(t * T + l * KISS_LANE));
            }
        }
        // k_kiss_pass<3>
        std::vector<unsigned char> arena(tot[1] + 1, 0xEE);
        std::vector<int> writes(tot[1] + 1, 0);
        for (long t = 0; t < ntiles; t++) {
            std::vector<unsigned> s_base(T, NOBASE);
            KissSum ex = tin[t];
            unsigned pk = toff[2 * t], by = toff[2 * t + 1];
            for (long l = 0; l < lanes; l++) {
                fends(t * T + l * KISS_LANE, ex, [&](const KissSum& run, long, const KissGap& g) {
                    const bool keep = g.kind == KISS_G_DELIVERED;
                    s_base[run.nfend - tin[t].nfend] = keep ? by : NOBASE;
                    if (keep) { pk += 1; by += g.len; }
                });
                ex = kiss_combine(ex, lane_sum(t * T + l * KISS_LANE));
            }
            KissSum run = tin[t];
            for (long v = t * T; v < (t + 1) * T && v < len; v++) {
                bool hn;
                unsigned rank, value;
                if (V[v] != KISS_FEND && run.last >= KISS_VIRT && kiss_emit(run, (int)v, v > 0 ? V[v - 1] : 0u, V[v], &rank, &value)) {
                    const unsigned kf = run.nfend - tin[t].nfend;
                    const unsigned base = kf < sums[t].nfend ? s_base[kf] : obase[slot(run.last)];
                    if (base != NOBASE) {
                        if (base + rank >= tot[1]) { std::printf("byte beyond the arena\n"); return 1; }
                        arena[base + rank] = (unsigned char)value;
                        writes[base + rank] += 1;
                    }
                }
                run = kiss_combine(run, at(v, 0, &hn));
            }
        }
        for (unsigned i = 0; i < tot[1]; i++)
            if (writes[i] != 1) { std::printf("arena byte %u has %d writers\n", i, writes[i]); return 1; }
        next.carry.assign(V.end() - ncarry, V.end());
        for (const Rec& r : recs) {
            std::printf("P %ld %ld %u %u ", push, r.pos, r.port, r.in_bytes);
            if (!r.len) std::printf("-");
            for (unsigned i = 0; i < r.len; i++) std::printf("%02x", arena[r.start + i]);
            std::printf("\n");
        }
        st = next;
        w0 += n;
        std::printf("S %llu %llu %llu %llu %llu\n", st.stats[0], st.stats[1], st.stats[2], st.stats[3], st.stats[4]);
    }
    return 0;
}
