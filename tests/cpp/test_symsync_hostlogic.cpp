// The host-only logic of rr_symbol_sync_create / _push / _push_dev / _produced (rustradio_amd/csrc/symsync_host.hpp), driven
// without a device: every refusal with its sentence, the stride arithmetic at its edges, the derived parameters, and the copy-out
// of the counts — fed hostile numbers above n, which must come out clamped — with guard elements behind `cap`.  Built with
// -fsanitize=address,undefined and run by tests/test_symsync_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/symsync_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static std::string str(const char* s) { return s ? s : ""; }

int main() {
    using namespace rr;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float two[2] = {0.0001f, 0.99999999f}, one[1] = {1.0f};
    float eight[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    // create-time checks
    CHECK(symsync_check(50000.0f / 9600.0f, 0.1f, two, 2, 1) == nullptr && symsync_check(4.0f, 1.0f, one, 1, 4096) == nullptr);
    CHECK(symsync_check(4.0f, 2.0f, eight, 8, 64) == nullptr && symsync_check(4.0f, 0.0f, one, 1, 1) == nullptr);
    for (float sps : {1.0f, 0.5f, 0.0f, -4.0f, nan, -inf})
        CHECK(str(symsync_check(sps, 0.1f, two, 2, 1)) == "sps must be above 1");
    CHECK(symsync_check(std::nextafter(1.0f, 2.0f), 0.0f, one, 1, 1) == nullptr);
    for (float dev : {-0.1f, 2.0001f, nan, inf, -inf})
        CHECK(str(symsync_check(4.0f, dev, two, 2, 1)) == "max_deviation out of range");
    CHECK(str(symsync_check(4.0f, 1.0f, nullptr, 2, 1)) == "SymbolSync needs 1 to 8 finite taps");
    CHECK(str(symsync_check(4.0f, 1.0f, two, 0, 1)) == "SymbolSync needs 1 to 8 finite taps");
    CHECK(str(symsync_check(4.0f, 1.0f, eight, 9, 1)) == "SymbolSync needs 1 to 8 finite taps");
    CHECK(str(symsync_check(4.0f, 1.0f, eight, ~(size_t)0, 1)) == "SymbolSync needs 1 to 8 finite taps");
    for (float bad : {nan, inf, -inf}) {
        float t[3] = {0.5f, bad, 0.5f};
        CHECK(str(symsync_check(4.0f, 1.0f, t, 3, 1)) == "SymbolSync needs 1 to 8 finite taps");
        CHECK(symsync_check(4.0f, 1.0f, t, 1, 1) == nullptr);              // (only the taps that count are looked at)
    }
    CHECK(str(symsync_check(4.0f, 1.0f, one, 1, 0)) == "nstreams out of range");
    CHECK(str(symsync_check(4.0f, 1.0f, one, 1, 4097)) == "nstreams out of range");
    CHECK(str(symsync_check(4.0f, 1.0f, one, 1, ~(size_t)0)) == "nstreams out of range");
    CHECK(str(symsync_check(nan, nan, nullptr, 0, 0)) == "sps must be above 1");       // the order of the sentences
    // the derived parameters, in the reference's operation order
    {
        const float sps = 50000.0f / 9600.0f, dev = 0.1f;
        const SyncParams p = symsync_params(sps, dev, two, 2);
        const float mi = sps - dev, mx = sps + dev;
        CHECK(p.ntaps == 2 && p.taps[0] == two[0] && p.taps[1] == two[1] && p.taps[2] == 0.0f);
        CHECK(p.mx == mx && p.t_lo == mi * 0.8f && p.t_hi == mx * 1.2f && p.c_lo == mi - sps && p.c_hi == mx - sps);
        SyncState s;
        sync_init(s, p);
        CHECK(s.clock == sps && s.stream_pos == 0.0f && s.last_sym_boundary_pos == 0.0f && s.next_sym_middle == sps / 2.0f && s.last_sign == 0);
        CHECK(s.hist[0] == sps && s.hist[1] == 0.0f);                         // fill(sps): ntaps - 1 copies of sps
    }
    // push-time checks and the stride edges
    {
        const float x = 0;
        float y = 0;
        CHECK(symsync_check_push(nullptr, 0, 0, nullptr, 0) == nullptr && symsync_check_push(&x, 1, 1, &y, 1) == nullptr);
        CHECK(symsync_check_push(&x, 10, 10, &y, 10) == nullptr && symsync_check_push(&x, 13, 10, &y, 15) == nullptr);
        CHECK(str(symsync_check_push(&x, 9, 10, &y, 10)) == "symbol sync: in_stride below n");
        CHECK(str(symsync_check_push(&x, 10, 10, &y, 9)) == "symbol sync: out_stride below n");
        CHECK(str(symsync_check_push(nullptr, 10, 10, &y, 10)) == "symbol sync: null buffer");
        CHECK(str(symsync_check_push(&x, 10, 10, nullptr, 10)) == "symbol sync: null buffer");
        const size_t big = (size_t)1 << 31;
        CHECK(symsync_check_push(&x, big, big - 1, &y, big) == nullptr);
        CHECK(str(symsync_check_push(&x, big, big, &y, big)) == "symbol sync: 2^31 samples or more in one push");
        CHECK(str(symsync_check_push(&x, ~(size_t)0, ~(size_t)0, &y, ~(size_t)0)) == "symbol sync: 2^31 samples or more in one push");
        CHECK(symsync_span(1, 100, 7) == 7 && symsync_span(3, 100, 7) == 207 && symsync_span(4096, 0, 0) == 0 && symsync_span(5, 9, 0) == 0);
        CHECK(symsync_span(2, 10, 10) == 20);
        CHECK(symsync_words(0) == 0 && symsync_words(1) == 1 && symsync_words(64) == 1 && symsync_words(65) == 2 && symsync_words(big - 1) == big / 64);
    }
    // the counts: hostile values above n come out as n; the copy-out never writes behind cap
    for (int round = 0; round < 200; round++) {
        const size_t ns = 1 + (size_t)round % 130, n = (size_t)round * 7 % 50;
        std::vector<unsigned long long> raw(ns);
        for (size_t c = 0; c < ns; c++) raw[c] = c % 3 == 0 ? ~0ull - c : (c % 3 == 1 ? n + c : c % (n + 1));
        std::vector<size_t> clean;
        symsync_clamp_counts(raw.data(), ns, n, clean);
        CHECK(clean.size() == ns);
        for (size_t c = 0; c < ns; c++) CHECK(clean[c] <= n && (raw[c] > n ? clean[c] == n : clean[c] == raw[c]));
        for (size_t cap : {(size_t)0, (size_t)1, ns - 1, ns, ns + 5}) {
            std::vector<size_t> out(cap + 2, 777);
            size_t total = 0;
            symsync_copy_counts(clean, cap ? out.data() : nullptr, cap, &total);
            CHECK(total == ns);
            for (size_t c = 0; c < cap + 2; c++) CHECK(out[c] == (c < cap && c < ns ? clean[c] : 777));
        }
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("symsync host logic ok\n");
    return 0;
}
