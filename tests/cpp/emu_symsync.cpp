// emu_symsync.cpp — rustradio_amd/csrc/symsync_core.hpp lane by lane on the CPU (g++ -O2 -ffp-contract=off): what k_sync_signs,
// k_sync_clock and k_sync_gather do to one stream, over the cases tests/test_symsync_cpu.py writes and holds to its model.
//   emu_symsync <cases file> <results file>
// cases:   i32 ncases; per case f32 sps, f32 max_deviation, i32 ntaps, f32 taps[8], i32 npushes, i32 len[npushes], f32 samples[sum len]
// results: per case and push i32 nwords, u64 words[nwords], i32 count, u32 idx[count], f32 clock[count], f32 syms[count],
//          f32 state[4], i32 last_sign, i32 nhist, f32 hist[nhist] (oldest first)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "symsync_host.hpp"

using namespace rr;

template <class T> static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short cases file\n"); exit(2); }
}
template <class T> static void wr(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: emu_symsync cases results\n"); return 2; }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int ncases = 0;
    rd(fi, &ncases, 1);
    for (int cs = 0; cs < ncases; cs++) {
        float sps, dev, taps[8];
        int ntaps, npushes;
        rd(fi, &sps, 1); rd(fi, &dev, 1); rd(fi, &ntaps, 1); rd(fi, taps, 8); rd(fi, &npushes, 1);
        std::vector<int> lens(npushes);
        rd(fi, lens.data(), lens.size());
        if (const char* e = symsync_check(sps, dev, taps, (size_t)ntaps, 1)) { fprintf(stderr, "case %d refused: %s\n", cs, e); return 1; }
        const SyncParams p = symsync_params(sps, dev, taps, (size_t)ntaps);
        SyncState st[2];                       // the Carried<> pair
        int cur = 0;
        sync_init(st[0], p);
        for (int len : lens) {
            std::vector<float> x(len);
            rd(fi, x.data(), x.size());
            const long n = len;
            // k_sync_signs: one word per wave
            const int nwords = (int)symsync_words((size_t)n);
            std::vector<unsigned long long> words(nwords);
            for (long w = 0; w < nwords; w++) words[w] = sync_sign_word(x.data(), n, w);
            // k_sync_clock: the lane of this stream
            std::vector<unsigned> idx(n ? n : 1);
            std::vector<float> clk(n ? n : 1), syms(n ? n : 1);
            int count = 0;
            if (n) {                           // (n == 0 launches nothing)
                SyncState s = st[cur];
                count = (int)sync_walk(s, p, words.data(), n, idx.data(), clk.data());
                st[cur ^ 1] = s;
                cur ^= 1;
            }
            // k_sync_gather
            for (int k = 0; k < count; k++) {
                if (idx[k] >= (unsigned)n) { fprintf(stderr, "index beyond the window\n"); return 1; }
                syms[k] = x[idx[k]];
            }
            wr(fo, &nwords, 1); wr(fo, words.data(), (size_t)nwords);
            wr(fo, &count, 1); wr(fo, idx.data(), (size_t)count); wr(fo, clk.data(), (size_t)count); wr(fo, syms.data(), (size_t)count);
            const SyncState& s = st[cur];
            const float four[4] = {s.clock, s.stream_pos, s.last_sym_boundary_pos, s.next_sym_middle};
            const int nh = ntaps - 1;
            float hist[8];
            for (int i = 0; i < nh; i++) hist[i] = s.hist[nh - 1 - i];
            wr(fo, four, 4); wr(fo, &s.last_sign, 1); wr(fo, &nh, 1); wr(fo, hist, (size_t)nh);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    printf("symsync core ok\n");
    return 0;
}
