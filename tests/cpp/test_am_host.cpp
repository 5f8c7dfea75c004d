// test_am_host.cpp — every refusal sentence of rr_am_demod's create and push, from rustradio_amd/csrc/am_host.hpp alone: no HIP, no
// library, no device (tests/test_am_cpu.py builds it with the host sanitizers).  Also the count rule and the host twin's refusal
// of a push leaving its state alone.
// Build: g++ -std=c++17 -ffp-contract=off -I rustradio_amd/csrc tests/cpp/test_am_host.cpp
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "am_host.hpp"

using namespace rr;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)
static bool says(const char* e, const char* what) { return e && std::strcmp(e, what) == 0; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> t3 = {0.25f, 0.5f, 0.25f}, big((size_t)AM_MAX_TAPS + 1, 0.0f), most((size_t)AM_MAX_TAPS, 0.0f);
    // create
    CHECK(am_check(2, t3.data(), 3, 12, 625, 1.0f) == nullptr);
    CHECK(am_check(4096, most.data(), most.size(), 1, 1, -2.0f) == nullptr);
    CHECK(says(am_check(0, t3.data(), 3, 1, 1, 1.0f), "nstreams out of range"));
    CHECK(says(am_check(4097, t3.data(), 3, 1, 1, 1.0f), "nstreams out of range"));
    CHECK(says(am_check(1, t3.data(), 0, 1, 1, 1.0f), "AmDemod needs 1 to 16384 finite taps"));
    CHECK(says(am_check(1, nullptr, 3, 1, 1, 1.0f), "AmDemod needs 1 to 16384 finite taps"));
    CHECK(says(am_check(1, big.data(), big.size(), 1, 1, 1.0f), "AmDemod needs 1 to 16384 finite taps"));
    { std::vector<float> b = t3; b[1] = nan; CHECK(says(am_check(1, b.data(), 3, 1, 1, 1.0f), "AmDemod needs 1 to 16384 finite taps")); }
    { std::vector<float> b = t3; b[2] = -inf; CHECK(says(am_check(1, b.data(), 3, 1, 1, 1.0f), "AmDemod needs 1 to 16384 finite taps")); }
    CHECK(says(am_check(1, t3.data(), 3, 1, 0, 1.0f), "RationalResampler created using deci 0"));
    CHECK(says(am_check(1, t3.data(), 3, 0, 1, 1.0f), "RationalResampler created using interp 0"));
    CHECK(says(am_check(1, t3.data(), 3, 0, 0, 1.0f), "RationalResampler created using deci 0"));
    CHECK(says(am_check(1, t3.data(), 3, ((size_t)1 << 31) + 1, 1, 1.0f), "am demod: reduced ratio part above 2^31"));
    CHECK(says(am_check(1, t3.data(), 3, 3, ((size_t)1 << 33) + 1, 1.0f), "am demod: reduced ratio part above 2^31"));
    CHECK(am_check(1, t3.data(), 3, (size_t)3 << 40, (size_t)7 << 40, 1.0f) == nullptr);          // 3 : 7 after the reduction
    CHECK(says(am_check(1, t3.data(), 3, 1, 1, nan), "scale must be finite"));
    CHECK(says(am_check(1, t3.data(), 3, 1, 1, inf), "scale must be finite"));
    // the geometry every legal shape gets fits the LDS the kernel asks for
    for (size_t L : {(size_t)1, (size_t)64, (size_t)289, (size_t)4097, (size_t)12045, (size_t)16384})
        for (size_t D : {(size_t)1, (size_t)7, (size_t)625, (size_t)1000, (size_t)1 << 31})
            for (size_t I : {(size_t)1, (size_t)12, (size_t)1 << 31}) {
                const AmGeom g = am_geom_of(L, I, D);
                CHECK(g.NG >= 1 && g.NG <= AM_NG_MAX && g.T == 32 * g.NG && g.KC % 64 == 0 && g.KC >= 64 && g.C == (int)L - 1);
                if (g.sparse) CHECK((long)g.T * g.KC <= (long)AM_LDS_FLOATS);
                else CHECK(am_span(g.T, g.I, g.D) + g.KC <= (long)AM_LDS_FLOATS);
            }
    // push
    float one = 0.0f;
    size_t k = 99;
    const AmGeom g = am_geom_of(3, 3, 7);
    CHECK(am_check_push(2, g, 0, &one, 7, 7, &one, 3, &k) == nullptr && k == 3);
    CHECK(says(am_check_push(2, g, 0, &one, 6, 7, &one, 3, &k), "am demod: in_stride below n") && k == 0);
    CHECK(says(am_check_push(2, g, 0, &one, 7, 7, &one, 2, &k), "am demod: out_stride below produced") && k == 0);
    CHECK(says(am_check_push(2, g, 0, nullptr, 7, 7, &one, 3, &k), "am demod: null buffer"));
    CHECK(says(am_check_push(2, g, 0, &one, 7, 7, nullptr, 3, &k), "am demod: null buffer"));
    CHECK(says(am_check_push(3, g, 0, &one, (size_t)1 << 29, (size_t)1 << 29, &one, (size_t)1 << 29, &k), "am demod: more than 2^30 samples in one push"));
    CHECK(says(am_check_push(1, g, 0, &one, ((size_t)1 << 30) + 1, ((size_t)1 << 30) + 1, &one, (size_t)1 << 30, &k), "am demod: more than 2^30 samples in one push"));
    CHECK(says(am_check_push(1, am_geom_of(3, 5, 2), 0, &one, (size_t)1 << 29, (size_t)1 << 29, &one, (size_t)1 << 31, &k), "am demod: more than 2^30 outputs in one push"));
    CHECK(says(am_check_push(4, am_geom_of(3, 2, 1), 0, &one, (size_t)1 << 27, (size_t)1 << 27, &one, (size_t)1 << 28, &k), "am demod: more than 2^30 outputs in one push") == false);
    CHECK(am_check_push(4096, g, 0, nullptr, 0, 0, nullptr, 0, &k) == nullptr && k == 0);          // an empty push needs no buffers
    CHECK(am_check_push(2, g, 6, &one, 1, 1, nullptr, 0, &k) == nullptr && k == 0);                // nor does one that produces nothing
    // the count rule: e after every push is ceil(N I / D) D - N I
    {
        long e = 0;
        unsigned long long N = 0, O = 0;
        const long I = 12, D = 625;
        for (long n : {1L, 0L, 52L, 53L, 624L, 625L, 1000000L, 7L}) {
            const long p = am_produced(e, n, I, D);
            e = am_next_e(e, n, p, I, D);
            N += (unsigned long long)n; O += (unsigned long long)p;
            CHECK(O == (N * I + D - 1) / D);
            CHECK(e >= 0 && e < D && (unsigned long long)e == O * D - N * I);
        }
    }
    // the host twin: a refused push throws its sentence and leaves the handle as it was
    {
        AmHost h(1, t3, 1, 1, 1.0f);
        std::vector<float> x = {3.0f, 4.0f, 0.0f, 1.0f}, y(2, -1.0f);
        CHECK(h.push(x.data(), 2, 2, y.data(), 2) == 2 && y[0] == 1.25f && y[1] == 2.75f);
        const long e0 = h.e; const unsigned long long t0 = h.total; const int c0 = h.cur;
        bool threw = false;
        try { h.push(x.data(), 1, 2, y.data(), 2); } catch (const char* e) { threw = says(e, "am demod: in_stride below n"); }
        CHECK(threw && h.e == e0 && h.total == t0 && h.cur == c0);
        bool refused = false;
        try { AmHost bad(1, t3, 1, 0, 1.0f); } catch (const char* e) { refused = says(e, "RationalResampler created using deci 0"); }
        CHECK(refused);
    }
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("am host ok\n");
    return 0;
}
