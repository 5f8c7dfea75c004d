// test_saver_host.cpp — BurstSaver and Delay of the C++ host mirror (rustradio_amd/host/rustradio.hpp) on one short stream.
// argv[1] names a file the Python test wrote: the stream, its cuts, and per window the PDUs rr.BurstSaver reported through the
// same library (tests/test_gpu_burst_saver.py holds those to the sequential models):
//   f32 alpha, f32 threshold, u64 delay, u64 max_size, u64 tail, u64 n, c32 x[n], u64 nwindows, then per window:
//   u64 len, u64 npdus, then per PDU: u64 stream_pos, u64 m, c32 samples[m]
// push() window by window must give exactly those PDUs, bit for bit; VectorSource -> Delay -> VectorSink under the mirror's Graph
// must give `delay` zeros and then the stream, with the source's tags moved `delay` samples on; the constructors' errors
// arrive as exceptions.
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_saver_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct WantPdu {
    uint64_t pos = 0;
    std::vector<Complex> samples;
};
struct Window {
    uint64_t len = 0;
    std::vector<WantPdu> pdus;
};
static bool same_bits(const std::vector<Complex>& a, const std::vector<Complex>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Complex)) == 0);
}
static bool has(const std::vector<Tag>& v, const Tag& t) { return std::find(v.begin(), v.end(), t) != v.end(); }

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s vectors.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Float alpha = 0, thr = 0;
    uint64_t delay = 0, max_size = 0, tail = 0, n = 0, nw = 0;
    bool ok = fread(&alpha, 4, 1, f) == 1 && fread(&thr, 4, 1, f) == 1 && fread(&delay, 8, 1, f) == 1 && fread(&max_size, 8, 1, f) == 1 &&
              fread(&tail, 8, 1, f) == 1 && fread(&n, 8, 1, f) == 1;
    std::vector<Complex> x(ok ? n : 0);
    ok = ok && fread(x.data(), 8, n, f) == n && fread(&nw, 8, 1, f) == 1;
    std::vector<Window> win(ok ? nw : 0);
    for (auto& w : win) {
        uint64_t np = 0;
        ok = ok && fread(&w.len, 8, 1, f) == 1 && fread(&np, 8, 1, f) == 1;
        if (!ok) break;
        w.pdus.resize(np);
        for (auto& p : w.pdus) {
            uint64_t m = 0;
            ok = ok && fread(&p.pos, 8, 1, f) == 1 && fread(&m, 8, 1, f) == 1;
            if (!ok) break;
            p.samples.resize(m);
            ok = ok && fread(p.samples.data(), 8, m, f) == m;
        }
    }
    fclose(f);
    if (!ok) { printf("short vector file\n"); return 2; }

    BurstSaver saver(alpha, thr, delay, max_size, tail);
    size_t at = 0, total = 0;
    for (const auto& w : win) {
        const std::vector<Complex> d(x.begin() + (long)at, x.begin() + (long)(at + w.len));
        at += w.len;
        std::vector<Float> env;
        auto a = saver.push(d, &env);
        CHECK(a.size() == w.pdus.size() && env.size() == d.size());
        for (size_t i = 0; i < w.pdus.size() && i < a.size(); i++) {
            CHECK(a[i].stream_pos == w.pdus[i].pos && same_bits(a[i].samples, w.pdus[i].samples));
            total++;
        }
    }
    CHECK(at == n && total >= 2);
    CHECK(saver.push({}).empty());

    // Delay under the Graph: zeros, then the stream; the source's tags sit `delay` samples on
    {
        const size_t dl = 37;
        const std::vector<Complex> head(x.begin(), x.begin() + (long)std::min<size_t>(n, 500));
        auto [src, s0] = VectorSource<Complex>::new_(head);
        auto [del, s1] = Delay<Complex>::new_(std::move(s0), dl);
        CHECK(std::string(del->block_name()) == "Delay");
        auto sink = std::make_unique<VectorSink<Complex>>(std::move(s1));
        auto hook = sink->hook();
        auto tags = sink->tag_hook();
        Graph g;
        g.add(std::move(src)); g.add(std::move(del)); g.add(std::move(sink));
        g.run();
        std::vector<Complex> want(dl, Complex(0, 0));
        want.insert(want.end(), head.begin(), head.end());
        CHECK(same_bits(*hook, want));
        CHECK(tags->size() == 3 && has(*tags, Tag(dl, "VectorSource::start", true)) && has(*tags, Tag(dl, "VectorSource::first", true)));
    }

    // the constructors' errors
    auto throws = [](auto&& make, const char* msg) {
        try { make(); } catch (const Error& e) { return std::string(e.what()) == msg; }
        return false;
    };
    CHECK(throws([] { BurstSaver b(1.5f, 0.5f, 1, 1, 1); }, "alpha out of range"));
    CHECK(throws([] { BurstSaver b(0.5f, 0.5f, 1, 512001, 1); }, "max_size beyond 512000 samples"));
    CHECK(throws([] { BurstSaver b(0.5f, 0.5f, 1024001, 1, 1); }, "delay: more than 1,024,000 samples"));
    CHECK(throws([] { auto [s, r] = VectorSource<Float>::new_(std::vector<Float>{1.0f}); Delay<Float>::new_(std::move(r), 1024001); },
                 "delay: more than 1,024,000 samples"));
    printf("%zu windows, %zu PDUs\n", win.size(), total);
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
