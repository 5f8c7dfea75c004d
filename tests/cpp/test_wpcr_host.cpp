// test_wpcr_host.cpp — Wpcr of the C++ host mirror (rustradio_amd/host/rustradio.hpp), the message form.  argv[1] names a file
// the Python test wrote from what rr.Wpcr(samp_rate) made of the same bursts through the same library:
//   f32 samp_rate, u64 nbursts, then per burst: u64 n, f32 x[n], f32 mid, u8 ok, u64 nsyms, f32 syms[nsyms], f32 sps, phase, frequency
// process() over the whole batch with the mids, and process_one() per burst where mid is 0, must give exactly those packets:
// the symbols bit for bit and the tags sps, phase, frequency at position 0 in the reference's order (wpcr.rs:187-194).
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_wpcr_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct Want {
    std::vector<Float> x, syms;
    Float mid = 0, sps = 0, phase = 0, frequency = 0;
    uint8_t ok = 0;
};
static bool same_bits(const std::vector<Float>& a, const std::vector<Float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Float)) == 0);
}
static void check_packet(const std::optional<Wpcr::Packet>& got, const Want& w) {
    CHECK(got.has_value() == (w.ok != 0));
    if (!got || !w.ok) return;
    CHECK(same_bits(got->first, w.syms));
    CHECK(got->second.size() == 3);
    if (got->second.size() != 3) return;
    CHECK(got->second[0] == Tag(0, "sps", w.sps));
    CHECK(got->second[1] == Tag(0, "phase", w.phase));
    CHECK(got->second[2] == Tag(0, "frequency", w.frequency));
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s vectors.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Float rate = 0;
    uint64_t nb = 0;
    bool ok = fread(&rate, 4, 1, f) == 1 && fread(&nb, 8, 1, f) == 1;
    std::vector<Want> want(ok ? nb : 0);
    for (auto& w : want) {
        uint64_t n = 0, ns = 0;
        ok = ok && fread(&n, 8, 1, f) == 1;
        if (!ok) break;
        w.x.resize(n);
        ok = ok && fread(w.x.data(), 4, n, f) == n && fread(&w.mid, 4, 1, f) == 1 && fread(&w.ok, 1, 1, f) == 1 && fread(&ns, 8, 1, f) == 1;
        if (!ok) break;
        w.syms.resize(ns);
        ok = ok && fread(w.syms.data(), 4, ns, f) == ns && fread(&w.sps, 4, 1, f) == 1 && fread(&w.phase, 4, 1, f) == 1 &&
             fread(&w.frequency, 4, 1, f) == 1;
    }
    fclose(f);
    if (!ok) { printf("short vector file\n"); return 2; }

    Wpcr wp(rate);
    std::vector<std::vector<Float>> bursts;
    std::vector<Float> mids;
    for (auto& w : want) { bursts.push_back(w.x); mids.push_back(w.mid); }
    auto got = wp.process(bursts, &mids);
    CHECK(got.size() == want.size());
    size_t valid = 0, dropped = 0;
    for (size_t b = 0; b < want.size() && b < got.size(); b++) {
        check_packet(got[b], want[b]);
        (want[b].ok ? valid : dropped)++;
        if (want[b].mid == 0.0f) check_packet(wp.process_one(want[b].x), want[b]);
    }
    CHECK(valid >= 2 && dropped >= 1);
    // without a sample rate there is no frequency tag
    Wpcr plain;
    for (auto& w : want)
        if (w.ok && w.mid == 0.0f) {
            auto p = plain.process_one(w.x);
            CHECK(p && p->second.size() == 2 && same_bits(p->first, w.syms));
            break;
        }
    // an empty batch, and the reference's None for a short burst
    CHECK(wp.process({}).empty());
    CHECK(!wp.process_one({1.0f, -1.0f, 1.0f}));
    printf("%zu bursts, %zu valid\n", want.size(), valid);
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
