// emu_fsk.cpp — rr_fsk_tx's host twin (fsk_host.hpp: FskHost over fsk_core.hpp's index maps and phase arithmetic) over case files
// that tests/fsk_model.py writes.  No HIP; tests/test_fsk_tx_cpu.py builds it with the host sanitizers.
//   emu_fsk cases.bin results.bin
// case:    i32 mode, i64 i1, i64 d1, f32 lo, f32 hi, f64 k1, f32 gain, i64 i2, i64 d2, f64 k2, i32 npushes, i64 lens[npushes], u8 bits[sum]
// result:  per push i64 n_audio, i64 n_out; then f32 audio[] (AFSK only) and c32 out[] of the whole case
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fsk_host.hpp"

template <class T> static T rd(FILE* f) {
    T v;
    if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: emu_fsk cases.bin results.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    const int ncases = rd<int32_t>(in);
    for (int c = 0; c < ncases; c++) {
        const int mode = rd<int32_t>(in);
        const int64_t i1 = rd<int64_t>(in), d1 = rd<int64_t>(in);
        const float lo = rd<float>(in), hi = rd<float>(in);
        const double k1 = rd<double>(in);
        const float gain = rd<float>(in);
        const int64_t i2 = rd<int64_t>(in), d2 = rd<int64_t>(in);
        const double k2 = rd<double>(in);
        if (const char* e = rr::fsk_check(mode, (size_t)i1, (size_t)d1, lo, hi, k1, gain, (size_t)i2, (size_t)d2, k2)) {
            fprintf(stderr, "case %d refused: %s\n", c, e);
            return 1;
        }
        const int np = rd<int32_t>(in);
        std::vector<int64_t> lens((size_t)np);
        size_t total = 0;
        for (auto& n : lens) { n = rd<int64_t>(in); total += (size_t)n; }
        std::vector<unsigned char> bits(total);
        if (total && fread(bits.data(), 1, total, in) != total) { fprintf(stderr, "short case file\n"); return 2; }
        rr::FskHost h(mode, (size_t)i1, (size_t)d1, lo, hi, k1, gain, (size_t)i2, (size_t)d2, k2);
        std::vector<std::complex<float>> o;
        std::vector<float> audio;
        size_t at = 0;
        for (int64_t n : lens) {
            const size_t o0 = o.size(), a0 = audio.size();
            // each push gets a buffer of exactly its bits: the sanitizer sees a read beyond them
            std::vector<unsigned char> mine(bits.begin() + (long)at, bits.begin() + (long)(at + (size_t)n));
            rr::FskPush u{};
            try { u = h.push(mine.data(), (size_t)n, o, mode == rr::FSK_AFSK ? &audio : nullptr); }
            catch (const char* e) { fprintf(stderr, "case %d: push refused: %s\n", c, e); return 1; }
            if (o.size() - o0 != (size_t)u.no || (mode == rr::FSK_AFSK && audio.size() - a0 != (size_t)u.na)) {
                fprintf(stderr, "case %d: a push made other counts than its plan\n", c);
                return 1;
            }
            const int64_t cnt[2] = {u.na, u.no};
            fwrite(cnt, sizeof cnt, 1, out);
            at += (size_t)n;
        }
        if (!audio.empty()) fwrite(audio.data(), sizeof(float), audio.size(), out);
        if (!o.empty()) fwrite(o.data(), sizeof(std::complex<float>), o.size(), out);
    }
    fclose(in);
    fclose(out);
    printf("fsk core ok\n");
    return 0;
}
