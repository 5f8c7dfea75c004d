// test_fsk_host.cpp — FskTx under the C++ host mirror (rustradio_amd/host/rustradio.hpp): fed the bits tests/test_gpu_fsk_tx_host_cpp.py
// wrote in the pushes it names; every audio sample and output goes back for the test to judge against tests/fsk_model.py.  Also
// the refusals in their own words, count() and the dims.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_fsk_host.cpp -L rustradio_amd/lib -lrustradio_amd
// in:  u64 mode, i1, d1, i2, d2, n, pushes; f32 lo, hi, gain; f64 k1, k2; u8 bits[n]; u64 len[pushes]
// out: per push u64 n_audio, n_out, f32 audio[n_audio] (AFSK), c32 out[n_out]
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
    uint64_t s[7] = {0};
    float lhg[3] = {0};
    double k[2] = {0};
    CHECK(rd(f, s, 7));
    CHECK(rd(f, lhg, 3));
    CHECK(rd(f, k, 2));
    const int mode = (int)s[0];
    const size_t n = s[5];
    std::vector<unsigned char> bits(n);
    std::vector<uint64_t> lens(s[6]);
    CHECK(rd(f, bits.data(), n));
    CHECK(rd(f, lens.data(), lens.size()));
    std::fclose(f);

    try { FskTx bad(7, s[1], s[2], lhg[0], lhg[1], k[0], lhg[2], s[3], s[4], k[1]); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "fsk tx: unknown mode")); }
    try { FskTx bad(mode, 0, s[2], lhg[0], lhg[1], k[0], lhg[2], s[3], s[4], k[1]); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "interpolation and decimation must be nonzero")); }

    FskTx tx(mode, s[1], s[2], lhg[0], lhg[1], k[0], lhg[2], s[3], s[4], k[1]);
    CHECK(tx.audio_tile() == 2048 && tx.out_tile() == 2048 && tx.scan_chunk_tiles() == 4096);
    if (mode == FskTx::Direct) {
        try { tx.push({1, 0, 1}, true); CHECK(false); }
        catch (const Error& e) { CHECK(std::strstr(e.what(), "DIRECT mode has no audio output")); }
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    uint64_t at = 0;
    for (uint64_t w : lens) {
        CHECK(at + w <= n);
        const std::vector<unsigned char> mine(bits.begin() + (long)at, bits.begin() + (long)(at + w));
        const auto want = tx.count(w);
        const auto p = tx.push(mine, mode == FskTx::Afsk);
        CHECK(p.out.size() == want.second);
        if (mode == FskTx::Afsk) CHECK(p.audio.size() == want.first);
        const uint64_t cnt[2] = {want.first, want.second};
        std::fwrite(cnt, sizeof cnt, 1, o);
        if (!p.audio.empty()) std::fwrite(p.audio.data(), sizeof(float), p.audio.size(), o);
        if (!p.out.empty()) std::fwrite(p.out.data(), sizeof(Complex), p.out.size(), o);
        at += w;
    }
    std::fclose(o);
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
