// test_am_mirror.cpp — AmDemod and AirspyDecode under the C++ host mirror (rustradio_amd/host/rustradio.hpp): fed the rows
// tests/test_gpu_am_host_cpp.py wrote in the windows it names; every output goes back for the test to judge against
// tests/am_model.py.  Also a refusal in the reference's words and the dims.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_am_mirror.cpp -L rustradio_amd/lib -lrustradio_amd
// in:  u64 nstreams, L, interp, deci, n, windows; f32 scale; f32 taps[L]; c32 x[nstreams][n]; u64 win[windows]
// out: per window u64 produced, f32 out[nstreams][produced]
#include <cstdio>
#include <cstring>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

template <class T> static bool rd(FILE* f, T* v, size_t n = 1) { return n == 0 || std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint64_t s[6] = {0};
    float scale = 0;
    CHECK(rd(f, s, 6));
    CHECK(rd(f, &scale, 1));
    const size_t ns = s[0], L = s[1], I = s[2], D = s[3], n = s[4];
    std::vector<float> taps(L);
    std::vector<Complex> x(ns * n);
    std::vector<uint64_t> win(s[5]);
    CHECK(rd(f, taps.data(), L));
    CHECK(rd(f, x.data(), ns * n));
    CHECK(rd(f, win.data(), win.size()));
    std::fclose(f);

    try { AmDemod bad(ns, taps, I, 0, scale); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "RationalResampler created using deci 0")); }

    {   // AirspyDecode of the mirror: I low, Q high, each / 1000; the source's start tag passes through
        auto [src, s0] = VectorSource<uint32_t>::new_({0x00010002u, 0xfffe03e8u, 0x80007fffu});
        src->work();
        auto [m, s1] = AirspyDecode::new_(std::move(s0));
        m->work();
        auto [o, tags] = s1.read_buf();
        CHECK(o.len() == 3 && o.slice()[0] == Complex(2.0f / 1000.0f, 1.0f / 1000.0f) && o.slice()[1] == Complex(1.0f, -2.0f / 1000.0f) &&
              o.slice()[2] == Complex(32767.0f / 1000.0f, -32768.0f / 1000.0f));
        CHECK(tags.size() >= 1 && tags[0].pos() == 0);
    }

    AmDemod d(ns, taps, I, D, scale);
    CHECK(d.nstreams() == ns && d.tile_outputs() >= 32 && d.tile_outputs() <= 192 && d.carry_samples() == L - 1);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    uint64_t at = 0;
    for (uint64_t w : win) {
        CHECK(at + w <= n);
        std::vector<std::vector<Complex>> rows(ns);
        for (size_t c = 0; c < ns; c++) rows[c].assign(x.begin() + (long)(c * n + at), x.begin() + (long)(c * n + at + w));
        const size_t want = d.count(w);
        const auto out = d.push(rows);
        CHECK(out.size() == ns);
        const uint64_t k = out.empty() ? 0 : out[0].size();
        CHECK(k == want);
        std::fwrite(&k, sizeof k, 1, o);
        for (size_t c = 0; c < ns; c++) {
            CHECK(out[c].size() == k);
            if (k) std::fwrite(out[c].data(), sizeof(float), k, o);
        }
        at += w;
    }
    std::fclose(o);
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
