// The host-only logic of rr_hdlc_framer_bound, rr_hdlc_framer_push_dev and rr_hdlc_framer_records
// (rustradio_amd/csrc/frame_host.hpp), driven without a device: the bound and its overflow, every refusal of a push, the
// descriptors a push uploads, the records made from the device's counters (and the counters it must not trust), the clamped
// copy-out — and many short-lived vectors, the handle churn of a test suite.  Built with -fsanitize=address,undefined and run by
// tests/test_frame_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/frame_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static std::string str(const char* s) { return s ? s : ""; }

int main() {
    using namespace rr;
    // create-time checks
    CHECK(frame_check_flags(0) == nullptr && frame_check_flags(15) == nullptr);
    CHECK(str(frame_check_flags(16)) == "unknown hdlc framer flags" && str(frame_check_flags(-1)) == "unknown hdlc framer flags");

    // the bound: 320 + 8 L + floor(8 L / 5)
    {
        const size_t lens[] = {0, 1, 2, 5, 256};
        CHECK(frame_bound(0, lens, 0) == 0);
        CHECK(frame_bound(0, lens, 1) == 320);
        CHECK(frame_bound(0, lens, 2) == 320 + 320 + 8 + 1);
        CHECK(frame_bound(RR_FRAME_FCS, lens, 1) == 320 + 16 + 3);
        CHECK(frame_bound(RR_FRAME_FCS | RR_FRAME_NRZI, lens, 5) ==
              5 * 320 + 8 * (2 + 3 + 4 + 7 + 258) + 16 / 5 + 24 / 5 + 32 / 5 + 56 / 5 + 2064 / 5);
        const size_t huge[] = {~(size_t)0, 1};
        CHECK(frame_bound(0, huge, 2) == ~(size_t)0 && frame_bound(RR_FRAME_FCS, huge, 1) == ~(size_t)0);
        const size_t half[] = {(~(size_t)0) / 16, (~(size_t)0) / 16};
        CHECK(frame_bound(0, half, 2) == ~(size_t)0);
    }
    // the refusals of a push, in the order they are made
    {
        size_t bound = 7;
        const size_t st[] = {0, 4, 4}, ln[] = {4, 2, 0};
        CHECK(frame_check_push(0, 6, st, ln, 3, 100000, &bound) == nullptr && bound == frame_bound(0, ln, 3));
        CHECK(frame_check_push(0, 6, st, ln, 0, 0, &bound) == nullptr && bound == 0);
        CHECK(frame_check_push(0, 6, nullptr, nullptr, 0, 0, &bound) == nullptr);
        CHECK(str(frame_check_push(0, 6, nullptr, ln, 3, 100000, &bound)) == "null packet descriptors");
        CHECK(str(frame_check_push(0, 5, st, ln, 3, 100000, &bound)) == "packet outside the buffer");
        const size_t st2[] = {7}, ln2[] = {0};
        CHECK(str(frame_check_push(0, 6, st2, ln2, 1, 100000, &bound)) == "packet outside the buffer");
        const size_t st3[] = {6};
        CHECK(frame_check_push(0, 6, st3, ln2, 1, 320, &bound) == nullptr);          // an empty packet at the very end
        const size_t st4[] = {~(size_t)0 - 1}, ln4[] = {4};                           // start + len wraps
        CHECK(str(frame_check_push(0, 6, st4, ln4, 1, 100000, &bound)) == "packet outside the buffer");
        CHECK(str(frame_check_push(0, 6, st, ln, 3, frame_bound(0, ln, 3) - 1, &bound)) == "output shorter than the framed bits can be");
        CHECK(frame_check_push(0, 6, st, ln, 3, frame_bound(0, ln, 3), &bound) == nullptr);
        // overlapping and repeated ranges are fine: the input is only read
        const size_t st5[] = {0, 0, 1}, ln5[] = {6, 6, 3};
        CHECK(frame_check_push(RR_FRAME_FCS, 6, st5, ln5, 3, 100000, &bound) == nullptr);
        // above 2^30 elements
        const size_t big = ((size_t)1 << 30) / 9;
        const size_t st6[] = {0}, ln6[] = {big};
        CHECK(str(frame_check_push(0, big, st6, ln6, 1, ~(size_t)0, &bound)) == "more than 2^30 framed bits in one push");
    }
    // the plan
    for (int flags : {0, (int)RR_FRAME_FCS}) {
        const size_t fcs = flags ? 2 : 0;
        const size_t st[] = {9, 0, 3, 3}, ln[] = {0, 128, 129, 1};
        FramePlan pl;
        frame_plan(flags, st, ln, 4, 128, pl);
        CHECK(pl.P == 4 && pl.words.size() == 3 * 4 + 2);
        CHECK(pl.starts()[0] == 9 && pl.starts()[3] == 3);
        CHECK(pl.pb()[0] == 0 && pl.pb()[1] == fcs && pl.pb()[2] == 128 + 2 * fcs && pl.pb()[4] == 258 + 4 * fcs && pl.nbytes == 258 + 4 * fcs);
        CHECK(pl.cpre()[0] == 0 && pl.cpre()[1] == 0 && pl.cpre()[2] == 1 && pl.cpre()[3] == 3 && pl.cpre()[4] == 4 && pl.nchunks == 4);
        FramePlan none;
        frame_plan(flags, nullptr, nullptr, 0, 128, none);
        CHECK(none.P == 0 && none.words.size() == 2 && none.nbytes == 0 && none.nchunks == 0);
    }
    // records from the device's counters, and counters that cannot be right
    for (int it = 0; it < 200; it++) {
        const int flags = it & 1 ? RR_FRAME_FCS : 0;
        const size_t fcs = flags ? 2 : 0, P = (size_t)(it % 7);
        std::vector<size_t> lens(P);
        std::vector<unsigned> cb(P + 1, 0u), crc(flags ? P : 0);
        size_t total = 0;
        for (size_t p = 0; p < P; p++) {
            lens[p] = (size_t)((it * 31 + p * 17) % 40);
            const unsigned stuffed = (unsigned)((8 * (lens[p] + fcs) / 5) * ((it + p) % 3) / 2);
            cb[p + 1] = cb[p] + stuffed;
            if (flags) crc[p] = 0x10000u + (unsigned)(p * 257 + it);                 // (bits above 16 are dropped)
            total += 320 + 8 * (lens[p] + fcs) + stuffed;
        }
        const size_t bound = frame_bound(flags, lens.data(), P);
        std::vector<rr_frame_record> rec;
        size_t produced = 99;
        CHECK(frame_records(flags, lens, cb, crc, total, bound, rec, &produced) == nullptr);
        CHECK(rec.size() == P && produced == total);
        size_t at = 0;
        for (size_t p = 0; p < P && p < rec.size(); p++) {
            CHECK(rec[p].start == at && rec[p].len == 320 + 8 * (lens[p] + fcs) + rec[p].stuffed && rec[p].stuffed == cb[p + 1] - cb[p]);
            CHECK(rec[p].fcs == (flags ? (unsigned short)(p * 257 + it) : 0));
            at += rec[p].len;
        }
        // copy-out: every cap around the size, NULL with cap 0, an exactly sized destination (an overrun is the sanitizer's)
        for (size_t cap = 0; cap <= P + 2; cap++) {
            std::vector<rr_frame_record> out(std::min(cap, P));                     // no slack
            size_t n = 99;
            frame_copy_out(rec, out.empty() ? nullptr : out.data(), cap, &n);
            CHECK(n == P);
            for (size_t k = 0; k < out.size(); k++) CHECK(out[k].start == rec[k].start && out[k].len == rec[k].len);
        }
        size_t n = 99;
        frame_copy_out(rec, nullptr, 0, &n);
        CHECK(n == P);
        if (!P) continue;
        // what must be refused: a total that is not the sum, counters that shrink or hold more than a packet can, a wrong size
        CHECK(frame_records(flags, lens, cb, crc, total + 1, bound, rec, &produced) != nullptr && rec.empty() && produced == 0);
        std::vector<unsigned> bad(cb);
        bad[P] = bad[P - 1] + (unsigned)(8 * (lens[P - 1] + fcs) / 5) + 1;
        CHECK(frame_records(flags, lens, bad, crc, total, ~(size_t)0, rec, &produced) != nullptr && rec.empty());
        bad = cb;
        bad[0] = 1;
        if (P > 0) bad[1] = std::max(bad[1], 1u);
        CHECK(frame_records(flags, lens, bad, crc, total, bound, rec, &produced) != nullptr);
        bad = cb;
        bad.pop_back();
        CHECK(frame_records(flags, lens, bad, crc, total, bound, rec, &produced) != nullptr);
        if (P > 1) {
            bad = cb;
            bad[P - 1] = bad[P] + 5;
            CHECK(frame_records(flags, lens, bad, crc, total, bound, rec, &produced) != nullptr);
        }
        if (flags) {
            std::vector<unsigned> shortcrc(crc.begin(), crc.end() - 1);
            CHECK(frame_records(flags, lens, cb, shortcrc, total, bound, rec, &produced) != nullptr);
        }
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("frame host logic ok\n");
    return 0;
}
