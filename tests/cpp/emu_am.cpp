// emu_am.cpp — rustradio_amd/csrc/am_core.hpp tile by tile and thread by thread on the CPU through the host twin of am_host.hpp
// (g++ -ffp-contract=off, with the host sanitizers in tests/test_am_cpu.py): what k_am does to nstreams streams over the pushes
// tests/am_model.py writes.
//   emu_am <cases file> <results file>
//   emu_am --dims L I D            prints "T C KC sparse" of the geometry (I, D, L) fix: what rr_am_demod_dims says on a device
// cases:   i32 ncases; per case i32 nstreams, i32 L, i64 interp, i64 deci, f32 scale, f32 taps[L], i32 npushes, i32 len[npushes],
//          then per push f32 samples[nstreams][len][2]
// results: per case and push i32 produced, f32 out[nstreams][produced]; every output buffer is filled with a sentinel first, and
//          an element beyond a count that no longer holds it ends the run
// Before the cases: what am_check_push refuses, in its words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "am_host.hpp"

using namespace rr;

template <class T> static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short cases file\n"); exit(2); }
}
template <class T> static void wr(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "--dims")) {
        const float one = 1.0f;
        const size_t L = (size_t)atoll(argv[2]), I = (size_t)atoll(argv[3]), D = (size_t)atoll(argv[4]);
        if (const char* e = am_check(1, &one, 1, I, D, 1.0f)) { fprintf(stderr, "%s\n", e); return 1; }
        if (L < 1 || L > (size_t)AM_MAX_TAPS) { fprintf(stderr, "taps out of range\n"); return 1; }
        const AmGeom g = am_geom_of(L, I, D);
        printf("%d %d %d %d\n", g.T, g.C, g.KC, g.sparse);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: emu_am cases results | emu_am --dims L I D\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    const unsigned SENT = 0x7fc12345u;
    {   // what a push refuses, and that an empty push needs no buffers
        float one = 0.0f;
        size_t k = 0;
        const AmGeom g = am_geom(3, 3, 7), up = am_geom(3, 5, 2);
        auto says = [](const char* e, const char* what) { return e && std::strstr(e, what); };
        if (!says(am_check_push(2, g, 0, &one, 6, 7, &one, 3, &k), "in_stride below n") ||
            !says(am_check_push(2, g, 0, &one, 7, 7, &one, 2, &k), "out_stride below produced") ||
            am_check_push(2, g, 0, &one, 7, 7, &one, 3, &k) || k != 3 ||
            !says(am_check_push(2, g, 0, nullptr, 7, 7, &one, 3, &k), "null buffer") ||
            !says(am_check_push(2, g, 0, &one, 7, 7, nullptr, 3, &k), "null buffer") ||
            am_check_push(2, g, 6, &one, 1, 1, nullptr, 0, &k) || k != 0 ||         // a push that produces nothing needs no output buffer
            !says(am_check_push(3, g, 0, &one, (size_t)1 << 29, (size_t)1 << 29, &one, (size_t)1 << 29, &k), "more than 2^30 samples") ||
            !says(am_check_push(1, up, 0, &one, (size_t)1 << 29, (size_t)1 << 29, &one, (size_t)1 << 31, &k), "more than 2^30 outputs") ||
            am_check_push(4096, g, 0, nullptr, 0, 0, nullptr, 0, &k) || k != 0) {
            fprintf(stderr, "push refusals\n");
            return 1;
        }
    }
    int ncases = 0;
    rd(fi, &ncases, 1);
    for (int cs = 0; cs < ncases; cs++) {
        int ns, L, npushes;
        long long interp, deci;
        float scale;
        rd(fi, &ns, 1); rd(fi, &L, 1); rd(fi, &interp, 1); rd(fi, &deci, 1); rd(fi, &scale, 1);
        if (ns < 1 || L < 1 || L > 1 << 20 || interp < 1 || deci < 1) { fprintf(stderr, "case %d: bad header\n", cs); return 2; }
        std::vector<float> taps((size_t)L);
        rd(fi, taps.data(), taps.size());
        rd(fi, &npushes, 1);
        std::vector<int> lens((size_t)npushes);
        rd(fi, lens.data(), lens.size());
        if (const char* e = am_check((size_t)ns, taps.data(), (size_t)L, (size_t)interp, (size_t)deci, scale)) {
            fprintf(stderr, "case %d refused: %s\n", cs, e);
            return 1;
        }
        AmHost h((size_t)ns, taps, (size_t)interp, (size_t)deci, scale);
        unsigned long long total = 0;
        auto O = [&](unsigned long long N) { return (N * (unsigned long long)h.g.I + (unsigned long long)h.g.D - 1) / (unsigned long long)h.g.D; };
        for (int len : lens) {
            const size_t n = (size_t)len, stride = n + 3;             // (a stride above n: the gap must stay untouched)
            const size_t want = (size_t)(O(total + n) - O(total)), ostride = want + 3;
            std::vector<float> x((size_t)ns * n * 2), in((size_t)ns * stride * 2, 0.0f), out((size_t)ns * ostride);
            rd(fi, x.data(), x.size());
            for (int c = 0; c < ns && n; c++) std::memcpy(in.data() + (size_t)c * stride * 2, x.data() + (size_t)c * n * 2, n * 2 * sizeof(float));
            for (auto& v : out) std::memcpy(&v, &SENT, 4);
            size_t produced = 0;
            try { produced = h.push(in.data(), stride, n, out.data(), ostride); }
            catch (const char* e) { fprintf(stderr, "case %d: push refused: %s\n", cs, e); return 1; }
            if (produced != want) { fprintf(stderr, "case %d: produced %zu, expected %zu\n", cs, produced, want); return 1; }
            total += n;
            const int k = (int)produced;
            wr(fo, &k, 1);
            for (int c = 0; c < ns; c++) {
                const float* row = out.data() + (size_t)c * ostride;
                for (size_t i = produced; i < ostride; i++)
                    if (std::memcmp(row + i, &SENT, 4) != 0) { fprintf(stderr, "case %d: written beyond the count\n", cs); return 1; }
                wr(fo, row, produced);
            }
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    printf("am core ok\n");
    return 0;
}
