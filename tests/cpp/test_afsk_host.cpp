// test_afsk_host.cpp — AfskDemod under the C++ host mirror (rustradio_amd/host/rustradio.hpp): fed the rows
// tests/test_gpu_afsk_host_cpp.py wrote in the windows it names; every output goes back for the test to judge against
// tests/afsk_model.py.  Also the refusal of an even Hilbert length in the reference's words, the dims, and AddConst of the mirror.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_afsk_host.cpp -L rustradio_amd/lib -lrustradio_amd
// in:  u64 nstreams, H, L, n, windows; f32 gain, offset; f32 taps[L]; f32 x[nstreams][n]; u64 win[windows]
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
    uint64_t s[5] = {0};
    float go[2] = {0};
    CHECK(rd(f, s, 5));
    CHECK(rd(f, go, 2));
    const size_t ns = s[0], H = s[1], L = s[2], n = s[3];
    std::vector<float> taps(L), x(ns * n);
    std::vector<uint64_t> win(s[4]);
    CHECK(rd(f, taps.data(), L));
    CHECK(rd(f, x.data(), ns * n));
    CHECK(rd(f, win.data(), win.size()));
    std::fclose(f);

    try { AfskDemod bad(ns, H + 1, 0, 0.0f, go[0], taps, go[1]); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "hilbert filter len must be odd and greater than 1")); }

    {   // AddConst of the mirror (add_const.rs:66-68): Float and Complex, the source's start tag passes through
        auto [src, s0] = VectorSource<Float>::new_({1.5f, -2.0f, 0.25f});
        src->work();
        auto [m, s1] = AddConst<Float>::new_(std::move(s0), 3.0f);
        m->work();
        auto [o, tags] = s1.read_buf();
        CHECK(o.len() == 3 && o.slice()[0] == 4.5f && o.slice()[1] == 1.0f && o.slice()[2] == 3.25f);
        CHECK(tags.size() >= 1 && tags[0].pos() == 0);
        auto [src2, c0] = VectorSource<Complex>::new_({{1, 0}, {0, -1}});
        src2->work();
        auto [mc, c1] = AddConst<Complex>::new_(std::move(c0), Complex(0.5f, 2.0f));
        mc->work();
        auto [oc, tc] = c1.read_buf();
        CHECK(oc.len() == 2 && oc.slice()[0] == Complex(1.5f, 2.0f) && oc.slice()[1] == Complex(0.5f, 1.0f));
    }

    AfskDemod d(ns, H, 0, 0.0f, go[0], taps, go[1]);
    CHECK(d.nstreams() == ns && d.tile_samples() == 2048 && d.carry_samples() == H + L);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    uint64_t at = 0;
    for (uint64_t w : win) {
        CHECK(at + w <= n);
        std::vector<std::vector<float>> rows(ns);
        for (size_t c = 0; c < ns; c++) rows[c].assign(x.begin() + (long)(c * n + at), x.begin() + (long)(c * n + at + w));
        const auto out = d.push(rows);
        CHECK(out.size() == ns);
        const uint64_t k = out.empty() ? 0 : out[0].size();
        CHECK(k == (at ? w : (w ? w - 1 : 0)));
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
