// test_fsk_multi_host.cpp — FskTxMulti under the C++ host mirror (rustradio_amd/host/rustradio.hpp): fed the rows and the counts
// tests/test_gpu_fsk_tx_multi_host_cpp.py wrote, push after push; every stream's audio and outputs go back for the test to compare
// with rr.FskTxMulti.  Also the refusals in their own words, bound(), counts(), positions() and the dims.  Needs a GPU.
// Build: g++ -O2 -std=c++17 -pthread tests/cpp/test_fsk_multi_host.cpp -L rustradio_amd/lib -lrustradio_amd
// in:  u64 mode, nstreams, i1, d1, i2, d2, n_cap, pushes; f32 lo, hi, gain; f64 k1, k2;
//      per push: u64 counts[nstreams], u8 rows[nstreams][n_cap]
// out: per push and stream u64 n_audio, n_out, f32 audio[n_audio] (AFSK), c32 out[n_out]
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
    uint64_t s[8] = {0};
    float lhg[3] = {0};
    double k[2] = {0};
    CHECK(rd(f, s, 8));
    CHECK(rd(f, lhg, 3));
    CHECK(rd(f, k, 2));
    const int mode = (int)s[0];
    const size_t N = s[1], n_cap = s[6], pushes = s[7];
    const bool afsk = mode == FskTx::Afsk;

    try { FskTxMulti bad(0, mode, s[2], s[3], lhg[0], lhg[1], k[0], lhg[2], s[4], s[5], k[1]); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "nstreams out of range")); }
    try { FskTxMulti bad(N, 7, s[2], s[3], lhg[0], lhg[1], k[0], lhg[2], s[4], s[5], k[1]); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "fsk tx: unknown mode")); }

    FskTxMulti tx(N, mode, s[2], s[3], lhg[0], lhg[1], k[0], lhg[2], s[4], s[5], k[1]);
    CHECK(tx.nstreams() == N);
    CHECK(tx.audio_tile() == 2048 && tx.out_tile() == 2048 && tx.scan_chunk_tiles() == 4096);
    CHECK(tx.bound(0) == std::make_pair((size_t)0, (size_t)0));
    const auto cap = tx.bound(n_cap);
    if (!afsk) {
        try { tx.push(std::vector<std::vector<unsigned char>>(N, {1, 0, 1}), {}, true); CHECK(false); }
        catch (const Error& e) { CHECK(std::strstr(e.what(), "fsk tx multi: DIRECT mode has no audio output")); }
    }
    try { tx.push(std::vector<std::vector<unsigned char>>(N + 1, {1, 0, 1})); CHECK(false); }
    catch (const Error& e) { CHECK(std::strstr(e.what(), "one row per stream")); }
    for (const auto& p : tx.positions()) CHECK(p.bits == 0 && p.audio == 0 && p.out == 0);      // (the refusals changed nothing)

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { printf("cannot open %s\n", argv[2]); return 2; }
    std::vector<unsigned long long> bits_total(N, 0), audio_total(N, 0), out_total(N, 0);
    for (size_t p = 0; p < pushes; p++) {
        std::vector<uint64_t> c64(N);
        CHECK(rd(f, c64.data(), N));
        std::vector<size_t> counts(c64.begin(), c64.end());
        std::vector<std::vector<unsigned char>> rows(N, std::vector<unsigned char>(n_cap));
        for (auto& r : rows) CHECK(rd(f, r.data(), n_cap));
        const auto made = tx.push(rows, counts, afsk);
        const auto cnt = tx.counts();
        CHECK(made.out.size() == N && cnt.size() == N);
        for (size_t c = 0; c < N; c++) {
            CHECK(made.out[c].size() == cnt[c].second && made.out[c].size() <= cap.second);
            if (afsk) CHECK(made.audio[c].size() == cnt[c].first && made.audio[c].size() <= cap.first);
            const uint64_t w[2] = {cnt[c].first, cnt[c].second};
            std::fwrite(w, sizeof w, 1, o);
            if (afsk && !made.audio[c].empty()) std::fwrite(made.audio[c].data(), sizeof(float), made.audio[c].size(), o);
            if (!made.out[c].empty()) std::fwrite(made.out[c].data(), sizeof(Complex), made.out[c].size(), o);
            bits_total[c] += std::min<size_t>(counts[c], n_cap);
            audio_total[c] += cnt[c].first;
            out_total[c] += cnt[c].second;
        }
    }
    std::fclose(f);
    std::fclose(o);
    const auto pos = tx.positions();
    CHECK(pos.size() == N);
    for (size_t c = 0; c < pos.size(); c++)
        CHECK(pos[c].bits == bits_total[c] && pos[c].audio == audio_total[c] && pos[c].out == out_total[c]);
    CHECK(tx.counts_dev() != nullptr);
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
