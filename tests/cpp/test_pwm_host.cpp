// test_pwm_host.cpp — PwmDecoder under the C++ host mirror (rustradio_amd/host/rustradio.hpp): built through its builder for the
// Complex stream of examples/restaurant_pager.rs, fed the samples tests/test_gpu_pwm_host_cpp.py wrote in the windows it names, then
// finish()ed; every frame goes back with its repeats and first_sample for the test to judge against tests/pwm_model.py.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_pwm_host.cpp -L rustradio_amd/lib -lrustradio_amd
#include <cstdio>
#include <cstring>

#include "../../rustradio_amd/host/rustradio.hpp"

using namespace rustradio;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

template <class T> static bool rd(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: %s samples.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    // short, long, frame_gap, reset_gap, frame_bits, min_repeats, delimiter, samples, windows
    uint64_t s[9] = {0};
    CHECK(rd(f, s, 9));
    std::vector<Complex> x(s[7]);
    std::vector<uint64_t> win(s[8]);
    if (s[7]) CHECK(rd(f, x.data(), s[7]));
    if (s[8]) CHECK(rd(f, win.data(), s[8]));
    std::fclose(f);

    // validate()'s refusals reach the caller in the reference's words, and Some(0) is one of them
    try { PwmDecoder<Float>::builder(0.0f, 2, 5, 9, 20).build(); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "high threshold must be finite")); }
    try { PwmDecoder<Float>::builder(0.5f, 2, 5, 9, 20).frame_bits(0).build(); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "fixed frame length must be greater than zero")); }

    auto d = PwmDecoder<Complex>::builder(0.5f, s[0], s[1], s[2], s[3]).frame_bits(s[4]).min_repeats(s[5])
                 .gap_pulse(s[6] ? PwmGapPulse::Delimiter : PwmGapPulse::Data).build<Complex>();
    CHECK(d.tile_samples() % 64 == 0);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    auto put = [&](const std::vector<PwmFrame>& frames, uint64_t push) {
        for (const PwmFrame& fr : frames) {
            CHECK(!fr.is_empty() && fr.len() == fr.bits().size());
            const uint64_t h[4] = {push, fr.first_sample(), fr.repeats(), fr.len()};
            std::fwrite(h, sizeof h, 1, o);
            std::fwrite(fr.bits().data(), 1, fr.len(), o);
        }
    };
    uint64_t at = 0, k = 0;
    for (uint64_t w : win) {
        CHECK(at + w <= x.size());
        put(d.push(std::vector<Complex>(x.begin() + (long)at, x.begin() + (long)(at + w))), k++);
        at += w;
    }
    put(d.finish(), k);
    try { d.push(std::vector<Complex>(4)); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "push after flush")); }
    std::fclose(o);
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
