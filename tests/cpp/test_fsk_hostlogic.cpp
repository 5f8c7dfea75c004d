// test_fsk_hostlogic.cpp — fsk_core.hpp's index arithmetic and fsk_host.hpp's refusals, with no device: the push-relative maps
// and the carried residues against brute force in 128-bit arithmetic from the stream's start, for random ratios (interpolating,
// decimating, 1:1, coprime parts near 2^31), random splits and carried positions near 2^62.  tests/test_fsk_tx_cpu.py builds it
// with the host sanitizers and runs it twice:
//   test_fsk_hostlogic                              the self-checks -> "fsk hostlogic ok"
//   test_fsk_hostlogic seek i1 d1 i2 d2 bits n      -> "audio out e1 e2 na no next_audio next_out next_e1 next_e2" of a push of n bits
//                                                    behind `bits` earlier ones (the test holds them against Python integers)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "fsk_host.hpp"

using namespace rr;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

static u128 cdiv(u128 a, u128 b) { return (a + b - 1) / b; }

// one stream: pushes of `lens` bits from position `start`; every map of every push against the definitions from the stream's start
static void walk_stream(const FskRatio& r1, const FskRatio& r2, unsigned long long start, const long* lens, int np, long probe) {
    FskPos p = fsk_seek(r1, r2, start);
    CHECK(p.e1 >= 0 && p.e1 < r1.D && p.e2 >= 0 && p.e2 < r2.D);
    CHECK((u128)p.audio == cdiv((u128)start * (u128)r1.I, (u128)r1.D));
    CHECK((u128)p.out == cdiv((u128)p.audio * (u128)r2.I, (u128)r2.D));
    for (int k = 0; k < np; k++) {
        const long n = lens[k];
        const FskPush u = fsk_plan(p, r1, r2, n);
        if (u.no < 0) break;                  // more audio than a push may make: nothing to compare
        const FskPos q = fsk_seek(r1, r2, p.bits + (unsigned long long)n);
        CHECK(u.next.bits == q.bits && u.next.audio == q.audio && u.next.out == q.out && u.next.e1 == q.e1 && u.next.e2 == q.e2);
        CHECK((unsigned long long)u.na == q.audio - p.audio && (unsigned long long)u.no == q.out - p.out);
        // a sample of the indices of the push (all of them when it is short): ends and a stride in between
        const long si = n > probe ? n / probe : 1;
        for (long i = 0; i <= n; i += (i + si > n && i < n) ? n - i : si) {
            const u128 g = cdiv((u128)(p.bits + (unsigned long long)i) * (u128)r1.I, (u128)r1.D);
            CHECK((u128)p.audio + (u128)fsk_first(r1, u.e1, i) == g);
            if (i < n) {
                CHECK(fsk_rep(r1, u.e1, i) == (long)(cdiv((u128)(p.bits + (unsigned long long)i + 1) * (u128)r1.I, (u128)r1.D) - g));
                FskWalk w = fsk_walk_first(r1, u.e1, i);
                CHECK(w.q == fsk_first(r1, u.e1, i));
                w.next();
                CHECK(w.q == fsk_first(r1, u.e1, i + 1));
            }
        }
        const long sm = u.na > probe ? u.na / probe : 1;
        for (long m = 0; m < u.na; m += (m + sm >= u.na && m < u.na - 1) ? u.na - 1 - m : sm) {
            const u128 gm = (u128)p.audio + (u128)m;
            const long b = fsk_src(r1, u.e1, m);
            CHECK(b >= 0 && b < n);
            CHECK((u128)p.bits + (u128)b == gm * (u128)r1.D / (u128)r1.I);
            FskWalk w = fsk_walk_src(r1, u.e1, m);
            CHECK(w.q == b);
            w.next();
            CHECK(w.q == fsk_src(r1, u.e1, m + 1));
            CHECK((u128)p.out + (u128)fsk_first(r2, u.e2, m) == cdiv(gm * (u128)r2.I, (u128)r2.D));
        }
        const long so = u.no > probe ? u.no / probe : 1;
        const long dq = ((long)FSK_B * r2.D) / r2.I, dr = ((long)FSK_B * r2.D) % r2.I;
        for (long o = 0; o < u.no; o += (o + so >= u.no && o < u.no - 1) ? u.no - 1 - o : so) {
            const u128 go = (u128)p.out + (u128)o;
            const long m = fsk_src(r2, u.e2, o);
            CHECK(m >= 0 && m < u.na);
            CHECK((u128)p.audio + (u128)m == go * (u128)r2.D / (u128)r2.I);
            // the map kernel's walk over FSK_B outputs at a time, and its place inside the run
            FskWalk w = fsk_walk(u.e2 + o * r2.D, dq, dr, r2.I);
            CHECK(w.q == m);
            const long j = (long)((unsigned)w.r / (unsigned)r2.D) + 1;
            CHECK(j == o - fsk_first(r2, u.e2, m) + 1);
            CHECK(j >= 1 && j <= fsk_rep(r2, u.e2, m));
            if (o + FSK_B < u.no) {
                w.next();
                CHECK(w.q == fsk_src(r2, u.e2, o + FSK_B));
                CHECK(w.r == (u.e2 + (o + FSK_B) * r2.D) % r2.I);
            }
        }
        p = u.next;
    }
}

static void self_checks() {
    std::mt19937_64 rng(20260);
    const long big[] = {2147483647L, 2147483648L, 2147483629L, 2147483587L, 2147483645L};
    const long pairs[][2] = {{10, 1}, {4, 1}, {40, 1}, {25, 24}, {3, 7}, {1, 1}, {7, 3}, {4099, 1}, {1, 4099}, {50, 1}, {5, 1}, {8, 1},
                             {2147483647L, 2147483648L}, {2147483648L, 2147483647L}, {2147483629L, 2147483587L}, {2147483648L, 1},
                             {1, 2147483648L}, {6, 4}, {1000, 10}};
    const int npairs = (int)(sizeof pairs / sizeof pairs[0]);
    for (int a = 0; a < npairs; a++)
        for (int b = 0; b < npairs; b++) {
            const FskRatio r1 = fsk_ratio(pairs[a][0], pairs[a][1]), r2 = fsk_ratio(pairs[b][0], pairs[b][1]);
            CHECK(fsk_gcd(r1.I, r1.D) == 1 && fsk_gcd(r2.I, r2.D) == 1);
            long lens[8];
            for (auto& n : lens) n = (long)(rng() % 97);
            lens[1] = 0; lens[2] = 1; lens[5] = 1; lens[6] = 2;
            walk_stream(r1, r2, 0, lens, 8, 1000);
            // longer pushes, probed; the audio stays below 2^30 where the first ratio interpolates by up to 2^31
            const long cap = r1.I > r1.D ? (long)(((u128)1 << 29) * (u128)r1.D / (u128)r1.I) : (1L << 29);
            long lens2[4];
            for (auto& n : lens2) n = cap > 1 ? (long)(rng() % (unsigned long long)cap) : cap;
            walk_stream(r1, r2, 0, lens2, 4, 64);
            // carried positions near 2^62 (of the bits; the refusal looks at the outputs, the arithmetic must hold either way)
            const unsigned long long far[] = {(1ull << 62) - 12345, (1ull << 61) + 7, (1ull << 40) + 1};
            for (unsigned long long s : far) {
                // keep audio and out inside 64 bits: positions scaled down by what the ratios multiply by
                u128 scale = ((u128)r1.qf + 1) * ((u128)r2.qf + 1);
                walk_stream(r1, r2, (unsigned long long)((u128)s / scale), lens, 8, 1000);
            }
        }
    for (long I : big)
        for (long D : big) {
            const FskRatio r = fsk_ratio(I, D), one = fsk_ratio(1, 1);
            long lens[3] = {1L << 30, 12345, 1};
            walk_stream(one, r, (1ull << 60), lens, 3, 64);
        }

    // the refusals, each its own sentence
    const double k = 0.001, nan = std::nan(""), inf = HUGE_VAL;
    const float fnan = std::nanf(""), finf = HUGE_VALF;
    auto is = [](const char* got, const char* want) { return got && std::string(got).find(want) != std::string::npos; };
    CHECK(fsk_check(FSK_AFSK, 10, 1, 1200, 2200, k, 0.5f, 4, 1, k) == nullptr);
    CHECK(fsk_check(FSK_DIRECT, 10, 1, -3000, 3000, k, 0.5f, 4, 1, nan) == nullptr);          // k2 is not looked at in DIRECT mode
    CHECK(is(fsk_check(2, 10, 1, 1, 2, k, 1, 4, 1, k), "unknown mode"));
    CHECK(is(fsk_check(-1, 10, 1, 1, 2, k, 1, 4, 1, k), "unknown mode"));
    CHECK(is(fsk_check(1, 0, 1, 1, 2, k, 1, 4, 1, k), "must be nonzero"));
    CHECK(is(fsk_check(1, 1, 0, 1, 2, k, 1, 4, 1, k), "must be nonzero"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, k, 1, 0, 1, k), "must be nonzero"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, k, 1, 1, 0, k), "must be nonzero"));
    CHECK(is(fsk_check(1, (1ul << 31) + 1, 1, 1, 2, k, 1, 1, 1, k), "above 2^31"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, k, 1, 2, (1ul << 31) + 1, k), "above 2^31"));
    CHECK(fsk_check(1, (1ul << 32), 2, 1, 2, k, 1, 1, 1, k) == nullptr);                       // 2^31 : 1 once reduced
    CHECK(is(fsk_check(1, ~(size_t)0, 1, 1, 2, k, 1, 1, 1, k), "above 2^31"));
    CHECK(is(fsk_check(1, 1, 1, fnan, 2, k, 1, 1, 1, k), "lo and hi"));
    CHECK(is(fsk_check(1, 1, 1, 1, finf, k, 1, 1, 1, k), "lo and hi"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, k, fnan, 1, 1, k), "gain must be finite"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, inf, 1, 1, 1, k), "k1 and k2"));
    CHECK(is(fsk_check(1, 1, 1, 1, 2, k, 1, 1, 1, nan), "k1 and k2"));

    const FskRatio r10 = fsk_ratio(10, 1), r4 = fsk_ratio(4, 1), r1 = fsk_ratio(1, 1), rbig = fsk_ratio(1L << 31, 1);
    const char some = 0;
    FskPos p0;
    FskPush u{};
    CHECK(fsk_check_push(FSK_AFSK, p0, r10, r4, &some, 3, &some, 120, &some, 30, &u) == nullptr && u.na == 30 && u.no == 120);
    CHECK(fsk_check_push(FSK_AFSK, p0, r10, r4, nullptr, 0, nullptr, 0, nullptr, 0, &u) == nullptr && u.na == 0 && u.no == 0);
    CHECK(is(fsk_check_push(FSK_DIRECT, p0, r10, r4, &some, 3, &some, 120, &some, 30, nullptr), "DIRECT mode has no audio"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r10, r4, nullptr, 3, &some, 120, nullptr, 0, nullptr), "null bit buffer"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r10, r4, &some, 3, nullptr, 120, nullptr, 0, nullptr), "null output buffer"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r10, r4, &some, 3, &some, 119, nullptr, 0, nullptr), "out_cap below"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r10, r4, &some, 3, &some, 120, &some, 29, nullptr), "audio_cap below"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r1, r1, &some, (1ul << 30) + 1, &some, ~(size_t)0, nullptr, 0, nullptr), "2^30 bits"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r10, r1, &some, 1ul << 30, &some, ~(size_t)0, nullptr, 0, nullptr), "2^30 audio samples"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r1, r4, &some, 1ul << 30, &some, ~(size_t)0, nullptr, 0, nullptr), "2^30 outputs"));
    CHECK(is(fsk_check_push(FSK_AFSK, p0, r1, rbig, &some, 1ul << 30, &some, ~(size_t)0, nullptr, 0, nullptr), "2^30 outputs"));
    CHECK(fsk_check_push(FSK_AFSK, p0, r1, r1, &some, 1ul << 30, &some, ~(size_t)0, nullptr, 0, &u) == nullptr && u.no == (1L << 30));
    FskPos far = fsk_seek(r1, r1, (1ull << 62) - 5);
    CHECK(fsk_check_push(FSK_AFSK, far, r1, r1, &some, 5, &some, 5, nullptr, 0, nullptr) == nullptr);
    CHECK(is(fsk_check_push(FSK_AFSK, far, r1, r1, &some, 6, &some, 6, nullptr, 0, nullptr), "beyond 2^62"));
}

int main(int argc, char** argv) {
    if (argc == 8 && !strcmp(argv[1], "seek")) {
        const FskRatio r1 = fsk_ratio(atol(argv[2]), atol(argv[3])), r2 = fsk_ratio(atol(argv[4]), atol(argv[5]));
        const FskPos p = fsk_seek(r1, r2, strtoull(argv[6], nullptr, 10));
        const FskPush u = fsk_plan(p, r1, r2, atol(argv[7]));
        printf("%llu %llu %ld %ld %ld %ld %llu %llu %ld %ld\n", p.audio, p.out, p.e1, p.e2, u.na, u.no, u.next.audio, u.next.out,
               u.next.e1, u.next.e2);
        return 0;
    }
    self_checks();
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    printf("fsk hostlogic ok\n");
    return 0;
}
