// test_pdu_host.cpp — StreamToPdu of the C++ host mirror (rustradio_amd/host/rustradio.hpp).  argv[1] names a file the Python
// test wrote: the stream, its cuts, and per window the PDUs of the sequential model (tests/pdu_model.py) with the offsets
// rr.StreamToPdu reported through the same library:
//   f32 threshold, u64 max_size, u64 tail, u64 n, f32 data[n], f32 trigger[n], u64 nwindows, then per window:
//   u64 len, u64 npdus, then per PDU: u64 stream_pos, u64 m, f32 samples[m], u8 has_mid, f32 mid
// push() window by window must give exactly those PDUs: positions, samples and offsets bit for bit; without Midpointer the
// same PDUs carry no offset; the errors of the constructor arrive as exceptions.
// Needs a GPU.  Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_pdu_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

struct WantPdu {
    uint64_t pos = 0;
    std::vector<Float> samples;
    uint8_t has_mid = 0;
    Float mid = 0;
};
struct Window {
    uint64_t len = 0;
    std::vector<WantPdu> pdus;
};
static bool same_bits(const std::vector<Float>& a, const std::vector<Float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Float)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: %s vectors.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    Float thr = 0;
    uint64_t max_size = 0, tail = 0, n = 0, nw = 0;
    bool ok = fread(&thr, 4, 1, f) == 1 && fread(&max_size, 8, 1, f) == 1 && fread(&tail, 8, 1, f) == 1 && fread(&n, 8, 1, f) == 1;
    std::vector<Float> data(ok ? n : 0), trig(ok ? n : 0);
    ok = ok && fread(data.data(), 4, n, f) == n && fread(trig.data(), 4, n, f) == n && fread(&nw, 8, 1, f) == 1;
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
            ok = ok && fread(p.samples.data(), 4, m, f) == m && fread(&p.has_mid, 1, 1, f) == 1 && fread(&p.mid, 4, 1, f) == 1;
        }
    }
    fclose(f);
    if (!ok) { printf("short vector file\n"); return 2; }

    StreamToPdu with(thr, max_size, tail, true), plain(thr, max_size, tail);
    size_t at = 0, total = 0, centred = 0;
    for (const auto& w : win) {
        const std::vector<Float> d(data.begin() + (long)at, data.begin() + (long)(at + w.len));
        const std::vector<Float> t(trig.begin() + (long)at, trig.begin() + (long)(at + w.len));
        at += w.len;
        auto a = with.push(d, t);
        auto b = plain.push(d, t);
        CHECK(a.size() == w.pdus.size() && b.size() == w.pdus.size());
        for (size_t i = 0; i < w.pdus.size() && i < a.size() && i < b.size(); i++) {
            const WantPdu& p = w.pdus[i];
            CHECK(a[i].stream_pos == p.pos && b[i].stream_pos == p.pos);
            CHECK(same_bits(a[i].samples, p.samples) && same_bits(b[i].samples, p.samples));
            CHECK(a[i].mid.has_value() == (p.has_mid != 0) && !b[i].mid.has_value());
            if (a[i].mid && p.has_mid) {
                CHECK(std::memcmp(&*a[i].mid, &p.mid, 4) == 0);
                auto c = a[i].centred();
                CHECK(c.size() == p.samples.size());
                for (size_t k = 0; k < c.size() && k < p.samples.size(); k++) CHECK(c[k] == p.samples[k] - p.mid);
                centred++;
            }
            CHECK(same_bits(b[i].centred(), p.samples));
            total++;
        }
        // the edges alternate and the windows' first one continues the previous window's last
        auto e = with.edges();
        for (size_t k = 1; k < e.size(); k++) CHECK(e[k].first > e[k - 1].first && e[k].second != e[k - 1].second);
    }
    CHECK(at == n && total >= 3 && centred >= 2);
    // an empty window reports nothing
    CHECK(with.push({}, {}).empty());
    // the constructor's errors
    bool threw = false;
    try { StreamToPdu bad(0.5f, 512001, 0); } catch (const Error& e) { threw = std::string(e.what()) == "max_size beyond 512000 samples"; }
    CHECK(threw);
    threw = false;
    try { with.push({1.0f}, {}); } catch (const Error&) { threw = true; }
    CHECK(threw);
    printf("%zu windows, %zu PDUs, %zu centred\n", win.size(), total, centred);
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
