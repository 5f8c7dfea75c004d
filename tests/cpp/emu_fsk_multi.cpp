// emu_fsk_multi.cpp — rr_fsk_tx_multi's host side (fsk_host.hpp: FskMultiHost, fsk_multi_bound, the refusals) on its own.  No HIP;
// tests/test_fsk_tx_multi_cpu.py builds it with the host sanitizers.
//   emu_fsk_multi             FskMultiHost per stream against FskHost, bit for bit, under ragged counts, counts above n_cap and
//                             zeros; fsk_multi_bound against the maximum of fsk_first over all residues -> "fsk multi ok"
//   emu_fsk_multi refusals    one line per case of the table below: "<label>|<sentence or ok>"
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fsk_host.hpp"

typedef std::vector<std::complex<float>> cvec;

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }

static const long SHAPES[5][4] = {{10, 1, 4, 1}, {40, 1, 25, 24}, {3, 7, 3, 7}, {7, 3, 4099, 1}, {1, 1, 1, 1}};
static const double K1 = 2.0 * 3.14159265358979323846 / 12000.0, K2 = 2.0 * 3.14159265358979323846 * 5000.0 / 48000.0;

template <class T> static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// N streams, three pushes of ragged counts: the multi twin against one FskHost per stream fed the clamped prefixes
static int check_twin(int mode, const long* sh) {
    const size_t N = 5, n_cap = 37, stride = 53;
    rr::FskMultiHost multi(N, mode, (size_t)sh[0], (size_t)sh[1], 1200.0f, 2200.0f, K1, 0.5f, (size_t)sh[2], (size_t)sh[3], K2);
    std::vector<rr::FskHost> one(N, rr::FskHost(mode, (size_t)sh[0], (size_t)sh[1], 1200.0f, 2200.0f, K1, 0.5f, (size_t)sh[2], (size_t)sh[3], K2));
    std::vector<cvec> mo(N), oo(N);
    std::vector<std::vector<float>> ma(N), oa(N);
    const unsigned long long COUNTS[3][5] = {{0, 1, n_cap, n_cap + 9, 20}, {n_cap, 0, 3, ~0ull, 1}, {5, n_cap + 1, 0, 0, n_cap}};
    for (int p = 0; p < 3; p++) {
        const unsigned long long* k = COUNTS[p];
        const size_t last = (size_t)(k[N - 1] < n_cap ? k[N - 1] : n_cap);
        // the last row ends with its count: the sanitizer sees a read beyond it; the other rows hold noise beyond theirs, which a
        // stream that read it would show in its samples
        std::vector<unsigned char> bits((N - 1) * stride + last);
        for (auto& b : bits) b = (unsigned char)((rnd() & 1) * (1 + rnd() % 255));
        const std::vector<rr::FskPush> u = multi.push(bits.data(), stride, n_cap, k, mo, mode == rr::FSK_AFSK ? &ma : nullptr);
        for (size_t c = 0; c < N; c++) {
            const size_t n = (size_t)(k[c] < n_cap ? k[c] : n_cap);
            std::vector<unsigned char> mine(bits.begin() + (long)(c * stride), bits.begin() + (long)(c * stride + n));
            const rr::FskPush w = one[c].push(mine.data(), n, oo[c], mode == rr::FSK_AFSK ? &oa[c] : nullptr);
            if (u[c].n != w.n || u[c].na != w.na || u[c].no != w.no || u[c].next.e1 != w.next.e1 || u[c].next.e2 != w.next.e2 ||
                u[c].next.bits != w.next.bits || u[c].next.audio != w.next.audio || u[c].next.out != w.next.out) {
                fprintf(stderr, "push %d stream %zu: other counts or positions than FskHost\n", p, c);
                return 1;
            }
            size_t ac = 0, oc = 0;
            rr::fsk_multi_bound(multi.s[c].r1, multi.s[c].r2, n_cap, &ac, &oc);
            if ((size_t)w.na > ac || (size_t)w.no > oc) { fprintf(stderr, "push %d stream %zu: beyond the bound\n", p, c); return 1; }
        }
    }
    for (size_t c = 0; c < N; c++) {
        if (!same_bits(mo[c], oo[c]) || !same_bits(ma[c], oa[c])) { fprintf(stderr, "stream %zu: other samples than FskHost\n", c); return 1; }
        if (multi.s[c].p1 != one[c].p1 || multi.s[c].p2 != one[c].p2) { fprintf(stderr, "stream %zu: other phases than FskHost\n", c); return 1; }
    }
    // an all-zero push and a push of no capacity change nothing
    const unsigned long long zeros[5] = {0, 0, 0, 0, 0};
    const unsigned char none = 0;
    const std::vector<cvec> before = mo;
    multi.push(&none, 0, n_cap, zeros, mo, mode == rr::FSK_AFSK ? &ma : nullptr);
    multi.push(&none, 0, 0, nullptr, mo, mode == rr::FSK_AFSK ? &ma : nullptr);
    for (size_t c = 0; c < N; c++)
        if (!same_bits(mo[c], before[c]) || multi.s[c].pos.bits != one[c].pos.bits || multi.s[c].pos.e1 != one[c].pos.e1) {
            fprintf(stderr, "stream %zu: an empty push changed something\n", c);
            return 1;
        }
    return 0;
}

// fsk_multi_bound against every pair of residues
static int check_bound(const long* sh) {
    const rr::FskRatio r1 = rr::fsk_ratio(sh[0], sh[1]), r2 = rr::fsk_ratio(sh[2], sh[3]);
    for (long n = 0; n <= 300; n += (n < 64 ? 1 : 59)) {
        long amax = 0, omax = 0;
        for (long e1 = 0; e1 < r1.D; e1++) {
            const long na = rr::fsk_first(r1, e1, n);
            if (na > amax) amax = na;
            for (long e2 = 0; e2 < r2.D; e2++) {
                const long no = rr::fsk_first(r2, e2, na);
                if (no > omax) omax = no;
            }
        }
        size_t ac = 0, oc = 0;
        rr::fsk_multi_bound(r1, r2, (size_t)n, &ac, &oc);
        if ((long)ac != amax || (long)oc != omax) {
            fprintf(stderr, "%ld:%ld-%ld:%ld n = %ld: bound (%zu, %zu), brute force (%ld, %ld)\n", sh[0], sh[1], sh[2], sh[3], n, ac, oc, amax, omax);
            return 1;
        }
    }
    return 0;
}

static void say(const char* label, const char* e) { printf("%s|%s\n", label, e ? e : "ok"); }

static int refusals() {
    const float nan = NAN, inf = INFINITY;
    const double dnan = NAN, dinf = INFINITY;
    const int A = rr::FSK_AFSK, D = rr::FSK_DIRECT;
    say("create ok", rr::fsk_multi_check(5, A, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create nstreams 0", rr::fsk_multi_check(0, A, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create nstreams 65535", rr::fsk_multi_check(65535, A, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create nstreams 65536", rr::fsk_multi_check(65536, A, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create mode", rr::fsk_multi_check(0, 2, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create interp1", rr::fsk_multi_check(0, A, 0, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create ratio", rr::fsk_multi_check(1, A, ((size_t)1 << 31) + 1, 1, 1200, 2200, K1, 0.5f, 4, 1, K2));
    say("create lo", rr::fsk_multi_check(1, A, 10, 1, nan, 2200, K1, 0.5f, 4, 1, K2));
    say("create hi", rr::fsk_multi_check(1, A, 10, 1, 1200, inf, K1, 0.5f, 4, 1, K2));
    say("create gain", rr::fsk_multi_check(1, A, 10, 1, 1200, 2200, K1, nan, 4, 1, K2));
    say("create k1", rr::fsk_multi_check(1, A, 10, 1, 1200, 2200, dinf, 0.5f, 4, 1, K2));
    say("create k2", rr::fsk_multi_check(1, A, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, dnan));
    say("create k2 direct", rr::fsk_multi_check(1, D, 10, 1, 1200, 2200, K1, 0.5f, 4, 1, dnan));
    const rr::FskRatio r1 = rr::fsk_ratio(10, 1), r2 = rr::fsk_ratio(4, 1);
    const char some = 0;
    const void* p = &some;
    const size_t big = (size_t)1 << 40;
    size_t ac = 0, oc = 0;
    say("push ok", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, p, 4000, p, 1000, &ac, &oc));
    if (ac != 1000 || oc != 4000) { fprintf(stderr, "push ok: bound (%zu, %zu)\n", ac, oc); return 1; }
    say("push ok no audio", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, p, 4000, nullptr, 0, nullptr, nullptr));
    say("push ok empty", rr::fsk_multi_check_push(A, 3, r1, r2, 0, nullptr, 0, 0, nullptr, 0, nullptr, 0, nullptr, nullptr));
    say("push direct audio", rr::fsk_multi_check_push(D, 3, r1, r2, 0, p, 100, 100, p, 4000, p, 1000, nullptr, nullptr));
    say("push bits_stride", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 99, 100, p, 4000, p, 1000, nullptr, nullptr));
    say("push out_stride", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, p, 3999, p, 1000, nullptr, nullptr));
    say("push audio_stride", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, p, 4000, p, 999, nullptr, nullptr));
    say("push audio_stride unused", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, p, 4000, nullptr, 0, nullptr, nullptr));
    say("push n_cap", rr::fsk_multi_check_push(A, 1, r1, r2, 0, p, big, ((size_t)1 << 30) + 1, p, big, nullptr, 0, nullptr, nullptr));
    say("push audio total", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, big, ((size_t)1 << 30) / 30 + 1, p, big, nullptr, 0, nullptr, nullptr));
    say("push out total", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, big, ((size_t)1 << 30) / 120 + 1, p, big, nullptr, 0, nullptr, nullptr));
    say("push out total fits", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, big, ((size_t)1 << 30) / 120, p, big, nullptr, 0, nullptr, nullptr));
    say("push null bits", rr::fsk_multi_check_push(A, 3, r1, r2, 0, nullptr, 100, 100, p, 4000, nullptr, 0, nullptr, nullptr));
    say("push null out", rr::fsk_multi_check_push(A, 3, r1, r2, 0, p, 100, 100, nullptr, 4000, nullptr, 0, nullptr, nullptr));
    say("push position", rr::fsk_multi_check_push(A, 3, r1, r2, ((unsigned long long)1 << 62) / 40 - 50, p, 100, 100, p, 4000, nullptr, 0, nullptr, nullptr));
    say("push position fits", rr::fsk_multi_check_push(A, 3, r1, r2, ((unsigned long long)1 << 62) / 40 - 100, p, 100, 100, p, 4000, nullptr, 0, nullptr, nullptr));
    const unsigned long long made[6] = {1000, 0, 7, 4000, 0, 28};
    say("counts ok", rr::fsk_multi_check_counts(made, 3, 1000, 4000));
    say("counts audio", rr::fsk_multi_check_counts(made, 3, 999, 4000));
    say("counts out", rr::fsk_multi_check_counts(made, 3, 1000, 3999));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "refusals")) return refusals();
    if (argc != 1) { fprintf(stderr, "usage: emu_fsk_multi [refusals]\n"); return 2; }
    for (const auto& sh : SHAPES) {
        for (int mode : {(int)rr::FSK_AFSK, (int)rr::FSK_DIRECT})
            if (check_twin(mode, sh)) return 1;
        if (check_bound(sh)) return 1;
    }
    printf("fsk multi ok\n");
    return 0;
}
