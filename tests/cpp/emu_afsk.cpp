// emu_afsk.cpp — rustradio_amd/csrc/afsk_core.hpp tile by tile and thread by thread on the CPU through the host twin of
// afsk_host.hpp (g++ -ffp-contract=off, with the host sanitizers in tests/test_afsk_cpu.py): what k_afsk does to nstreams streams
// over the pushes tests/afsk_model.py writes.
//   emu_afsk <cases file> <results file>
// cases:   i32 ncases; per case i32 nstreams, i32 H, i32 L, f32 gain, f32 offset, f32 hil[H], f32 taps[L], i32 npushes,
//          i32 len[npushes], then per push f32 samples[nstreams][len]
// results: per case and push i32 produced, f32 out[nstreams][produced]; every output buffer is filled with a sentinel first, and
//          an element beyond a count that no longer holds it ends the run
// Before the cases: what afsk_check_push refuses, in its words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "afsk_host.hpp"

using namespace rr;

template <class T> static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short cases file\n"); exit(2); }
}
template <class T> static void wr(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: emu_afsk cases results\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    const unsigned SENT = 0x7fc12345u;
    {   // what a push refuses, and that an empty push needs no buffers
        float one = 0.0f;
        auto says = [](const char* e, const char* what) { return e && std::strstr(e, what); };
        if (!says(afsk_check_push(2, &one, 3, 4, &one, 4), "in_stride below n") || !says(afsk_check_push(2, &one, 4, 4, &one, 3), "out_stride below n") ||
            !says(afsk_check_push(2, nullptr, 4, 4, &one, 4), "null buffer") || !says(afsk_check_push(2, &one, 4, 4, nullptr, 4), "null buffer") ||
            !says(afsk_check_push(3, &one, (size_t)1 << 29, (size_t)1 << 29, &one, (size_t)1 << 29), "more than 2^30 samples") ||
            !says(afsk_check_push(1, &one, ((size_t)1 << 30) + 1, ((size_t)1 << 30) + 1, &one, ((size_t)1 << 30) + 1), "more than 2^30 samples") ||
            afsk_check_push(4096, nullptr, 0, 0, nullptr, 0) || afsk_check_push(1, &one, (size_t)1 << 30, (size_t)1 << 30, &one, (size_t)1 << 30)) {
            fprintf(stderr, "push refusals\n");
            return 1;
        }
    }
    int ncases = 0;
    rd(fi, &ncases, 1);
    for (int cs = 0; cs < ncases; cs++) {
        int ns, H, L, npushes;
        float gain, offset;
        rd(fi, &ns, 1); rd(fi, &H, 1); rd(fi, &L, 1); rd(fi, &gain, 1); rd(fi, &offset, 1);
        if (ns < 1 || H < 1 || L < 1 || H > 1 << 20 || L > 1 << 20) { fprintf(stderr, "case %d: bad header\n", cs); return 2; }
        std::vector<float> hil((size_t)H), taps((size_t)L);
        rd(fi, hil.data(), hil.size()); rd(fi, taps.data(), taps.size());
        rd(fi, &npushes, 1);
        std::vector<int> lens((size_t)npushes);
        rd(fi, lens.data(), lens.size());
        if (const char* e = afsk_check((size_t)ns, (size_t)H, 0, 0.0f, gain, taps.data(), (size_t)L, offset)) {
            fprintf(stderr, "case %d refused: %s\n", cs, e);
            return 1;
        }
        AfskHost h((size_t)ns, hil, gain, taps, offset);
        unsigned long long total = 0;
        for (int len : lens) {
            const size_t n = (size_t)len, stride = n + 3;             // (a stride above n: the gap must stay untouched)
            std::vector<float> x((size_t)ns * n), in((size_t)ns * stride, 0.0f), out((size_t)ns * stride);
            rd(fi, x.data(), x.size());
            for (int c = 0; c < ns && n; c++) std::memcpy(in.data() + (size_t)c * stride, x.data() + (size_t)c * n, n * sizeof(float));
            for (auto& v : out) std::memcpy(&v, &SENT, 4);
            size_t produced = 0;
            try { produced = h.push(in.data(), stride, n, out.data(), stride); }
            catch (const char* e) { fprintf(stderr, "case %d: push refused: %s\n", cs, e); return 1; }
            const unsigned long long after = total + n;
            const size_t want = (size_t)((after ? after - 1 : 0) - (total ? total - 1 : 0));
            if (produced != want) { fprintf(stderr, "case %d: produced %zu, expected %zu\n", cs, produced, want); return 1; }
            total = after;
            const int k = (int)produced;
            wr(fo, &k, 1);
            for (int c = 0; c < ns; c++) {
                const float* row = out.data() + (size_t)c * stride;
                for (size_t i = produced; i < stride; i++)
                    if (std::memcmp(row + i, &SENT, 4) != 0) { fprintf(stderr, "case %d: written beyond the count\n", cs); return 1; }
                wr(fo, row, produced);
            }
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    printf("afsk core ok\n");
    return 0;
}
