// test_kiss_hostlogic.cpp — rustradio_amd/csrc/kiss_host.hpp without a device: the refusals, the plans, the descriptors, the
// validation of numbers a device might have written, and the clamped copy-out.  A stand-alone program: tests/test_kiss_cpu.py builds
// it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/kiss_host.hpp"

using namespace rr;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)
static bool says(const char* e, const char* what) { return e && std::strstr(e, what) != nullptr; }

static rr_kiss_packet pk(unsigned long long pos, unsigned long long start, unsigned len, unsigned in_bytes, unsigned port = 0) {
    rr_kiss_packet p{};
    p.pos = pos; p.start = start; p.len = len; p.in_bytes = in_bytes; p.port = port; p.reserved = 0;
    return p;
}

int main() {
    // ---- decode: create and push refusals, all "kiss decode: ..." ------------------------------------------------------------------------
    CHECK(says(kiss_check_create(0), "kiss decode: max_len out of range"));
    CHECK(says(kiss_check_create(((size_t)1 << 20) + 1), "kiss decode: max_len out of range"));
    CHECK(!kiss_check_create(1) && !kiss_check_create(10000) && !kiss_check_create((size_t)1 << 20));
    unsigned char one = 0;
    CHECK(!kiss_check_push(nullptr, 0) && !kiss_check_push(&one, 1) && !kiss_check_push(&one, (size_t)1 << 30));
    CHECK(says(kiss_check_push(nullptr, 1), "kiss decode: null input"));
    CHECK(says(kiss_check_push(&one, ((size_t)1 << 30) + 1), "kiss decode: more than 2^30 bytes"));
    // ---- decode: plans -----------------------------------------------------------------------------------------------------------------
    {
        const KissPlan p = kiss_plan(0, 1);
        CHECK(p.nv_max == 1 && p.ntiles == 1 && p.rec_cap == 0 && p.arena_cap == 1);
        const KissPlan q = kiss_plan(10000, 4096);
        CHECK(q.nv_max == 14096 && q.ntiles == 4 && q.rec_cap == 4096 && q.arena_cap == 14096);
        const KissPlan r = kiss_plan(3, 4093);
        CHECK(r.ntiles == 1 && r.rec_cap == 2048);
        CHECK(kiss_plan(1, 4096).ntiles == 2);
        CHECK(kiss_next_carry(0, 5, 10000) == 5 && kiss_next_carry(9999, 5, 10000) == 10000 && kiss_next_carry(3, 0, 2) == 2);
        // the largest push: every size fits 31 bits, as the kernels' int indices need
        const KissPlan big = kiss_plan((size_t)1 << 20, (size_t)1 << 30);
        CHECK(big.nv_max < ((size_t)1 << 31) && big.ntiles == (big.nv_max + 4095) / 4096);
    }
    // ---- decode: hostile counts and records ----------------------------------------------------------------------------------------------
    {
        const KissPlan p = kiss_plan(4, 20);              // window [100, 120), at most 4 carried bytes
        unsigned long long k[2] = {12, 24};
        CHECK(!kiss_check_count(k, p));
        k[0] = 13;
        CHECK(says(kiss_check_count(k, p), "more packets"));
        k[0] = 0; k[1] = 25;
        CHECK(says(kiss_check_count(k, p), "more packet bytes"));
        const unsigned long long b0[5] = {5, 3, 1, 1, 2};
        auto val = [&](const std::vector<rr_kiss_packet>& r, unsigned long long bytes, const unsigned long long* now) {
            return kiss_validate(r, p, 10, 100, 20, 4, bytes, b0, now);
        };
        const unsigned long long n2[5] = {7, 5, 1, 1, 2};
        std::vector<rr_kiss_packet> good = {pk(102, 0, 4, 5), pk(110, 4, 0, 0)};
        CHECK(!val(good, 4, n2));
        CHECK(!val({}, 0, b0));
        auto r = good;
        r[0].pos = 99;
        CHECK(says(val(r, 4, n2), "outside the push"));
        r = good; r[1].pos = 120;
        CHECK(says(val(r, 4, n2), "outside the push"));
        r = good; r[0].in_bytes = 10; r[0].len = 10;
        CHECK(says(val(r, 10, n2), "lengths out of range"));
        r = good; r[0].len = 6;
        CHECK(says(val(r, 6, n2), "lengths out of range"));
        r = good; r[0].len = 1;                           // four of five bytes escapes
        CHECK(says(val(r, 1, n2), "lengths out of range"));
        r = good; r[0].in_bytes = 7; r[0].len = 7;        // 8 bytes of gap, 2 of the window and 4 carried in front of pos
        CHECK(says(val(r, 7, n2), "overlap or run backwards"));
        r = good; r[1].pos = 102;
        CHECK(says(val(r, 4, n2), "overlap or run backwards"));
        r = good; r[1].pos = 103;                         // no room for the port byte behind the first packet's FEND
        CHECK(says(val(r, 4, n2), "overlap or run backwards"));
        r = good; r[1].start = 3;
        CHECK(says(val(r, 4, n2), "not packed"));
        r = good; r[0].port = 16;
        CHECK(says(val(r, 4, n2), "port out of range"));
        r = good; r[0].reserved = 1;
        CHECK(says(val(r, 4, n2), "port out of range"));
        CHECK(says(val(good, 5, n2), "arena bytes disagree"));
        const unsigned long long back[5] = {7, 5, 1, 0, 2};
        CHECK(says(val(good, 4, back), "ran backwards"));
        const unsigned long long off[5] = {7, 4, 2, 1, 2};
        CHECK(says(val(good, 4, off), "counters disagree"));
        const unsigned long long sum[5] = {8, 5, 1, 1, 2};
        CHECK(says(val(good, 4, sum), "counters disagree"));
        const unsigned long long many[5] = {5 + 21, 3, 1 + 21, 1, 2};
        CHECK(says(val({}, 0, many), "counters disagree"));
        std::vector<rr_kiss_packet> crowd(13, pk(101, 0, 0, 0));
        CHECK(says(val(crowd, 0, n2), "counts beyond the push"));
    }
    // ---- copy-out: the contract of rr_wpcr_results ---------------------------------------------------------------------------------------
    {
        std::vector<rr_kiss_packet> r = {pk(1, 0, 1, 1), pk(5, 1, 2, 2), pk(9, 3, 0, 0)};
        size_t total = 99;
        kiss_copy_out<rr_kiss_packet>(r, nullptr, 0, &total);
        CHECK(total == 3);
        std::vector<rr_kiss_packet> out(2);
        kiss_copy_out(r, out.data(), 2, &total);
        CHECK(total == 3 && out[1].pos == 5);
        std::vector<rr_kiss_packet> wide(5);
        kiss_copy_out(r, wide.data(), 5, &total);
        CHECK(total == 3 && wide[2].pos == 9 && wide[3].pos == 0);
    }
    // ---- encode: the bound and the refusals, all "kiss encode: ..." ----------------------------------------------------------------------
    {
        const size_t big = ~(size_t)0;
        const size_t l3[3] = {0, 5, 1};
        CHECK(kiss_encode_bound(nullptr, 0) == 0 && kiss_encode_bound(l3, 3) == 3 + 13 + 5);
        const size_t huge[2] = {big / 2, big / 2};
        CHECK(kiss_encode_bound(huge, 2) == big && kiss_encode_bound(huge, 1) == big);
        const size_t half[2] = {(big - 3) / 2, 0};
        CHECK(kiss_encode_bound(half, 1) == 3 + 2 * ((big - 3) / 2) && kiss_encode_bound(half, 2) == big);
        size_t bound = 7;
        size_t st[2] = {0, 3}, ln[2] = {3, 2};
        CHECK(!kiss_encode_check_push(5, st, ln, 2, 16, &bound) && bound == 16);
        CHECK(!kiss_encode_check_push(0, nullptr, nullptr, 0, 0, &bound) && bound == 0);
        CHECK(says(kiss_encode_check_push(5, nullptr, ln, 2, 16, &bound), "kiss encode: null packet descriptors"));
        CHECK(says(kiss_encode_check_push(5, st, nullptr, 2, 16, &bound), "kiss encode: null packet descriptors"));
        CHECK(says(kiss_encode_check_push(5, st, ln, 2, 15, &bound), "kiss encode: output shorter") && bound == 16);
        CHECK(says(kiss_encode_check_push(4, st, ln, 2, 16, &bound), "kiss encode: packet outside the buffer"));
        size_t far[1] = {6}, none[1] = {0};
        CHECK(says(kiss_encode_check_push(5, far, none, 1, 16, &bound), "kiss encode: packet outside the buffer"));
        size_t wrap[1] = {big};
        CHECK(says(kiss_encode_check_push(5, st, wrap, 1, big, &bound), "kiss encode: packet outside the buffer"));
        CHECK(says(kiss_encode_check_push(((size_t)1 << 30) + 1, st, ln, 2, 16, &bound), "kiss encode: more than 2^30 bytes"));
        // repeated ranges are fine, and their bound can pass 2^30 though the buffer does not
        const size_t n = (size_t)1 << 29;
        size_t st3[3] = {0, 0, 0}, ln3[3] = {n, n, n};
        CHECK(says(kiss_encode_check_push(n, st3, ln3, 3, big, &bound), "kiss encode: more than 2^30 encoded bytes"));
        size_t ln1[1] = {((size_t)1 << 29) - 2};
        CHECK(!kiss_encode_check_push(n, st3, ln1, 1, (size_t)1 << 30, &bound) && bound == ((size_t)1 << 30) - 1);
    }
    // ---- encode: descriptors and records ------------------------------------------------------------------------------------------------
    {
        size_t st[3] = {7, 0, 7}, ln[3] = {2, 0, 3};
        unsigned po[3] = {1, 12, 99};
        KissEncPlan pl;
        kiss_encode_plan(st, ln, po, 3, pl);
        CHECK(pl.P == 3 && pl.nbytes == 5 && pl.words.size() == 10);
        const unsigned long long want[10] = {7, 0, 7, 0, 2, 2, 5, 1, 12, 99};
        CHECK(std::memcmp(pl.words.data(), want, sizeof want) == 0);
        kiss_encode_plan(st, ln, nullptr, 3, pl);
        CHECK(pl.words[7] == 0 && pl.words[8] == 0 && pl.words[9] == 0);
        kiss_encode_plan(nullptr, nullptr, nullptr, 0, pl);
        CHECK(pl.P == 0 && pl.nbytes == 0 && pl.words.size() == 1);

        const std::vector<size_t> lens = {2, 0, 3};
        const std::vector<unsigned> ports = {1, 12, 99};
        std::vector<rr_kiss_frame_record> rec;
        size_t produced = 9;
        CHECK(!kiss_encode_records(lens, ports, {0, 1, 1, 4}, 18, 19, rec, &produced));
        CHECK(produced == 18 && rec.size() == 3 && rec[0].start == 0 && rec[0].len == 6 && rec[0].escaped == 1 && rec[0].port == 1);
        CHECK(rec[1].start == 6 && rec[1].len == 3 && rec[1].port == 12 && rec[2].start == 9 && rec[2].len == 9 && rec[2].escaped == 3 && rec[2].port == 0);
        CHECK(says(kiss_encode_records(lens, ports, {0, 1, 1}, 18, 19, rec, &produced), "counters of another push") && rec.empty() && produced == 0);
        CHECK(says(kiss_encode_records(lens, ports, {1, 1, 1, 4}, 18, 19, rec, &produced), "in front of the first packet"));
        CHECK(says(kiss_encode_records(lens, ports, {0, 3, 3, 4}, 18, 19, rec, &produced), "beyond what the packet can hold"));
        CHECK(says(kiss_encode_records(lens, ports, {0, 1, 0, 3}, 17, 19, rec, &produced), "beyond what the packet can hold"));
        CHECK(says(kiss_encode_records(lens, ports, {0, 1, 2, 4}, 18, 19, rec, &produced), "beyond what the packet can hold"));
        CHECK(says(kiss_encode_records(lens, ports, {0, 1, 1, 4}, 17, 19, rec, &produced), "beyond the bound"));
        CHECK(says(kiss_encode_records(lens, ports, {0, 1, 1, 4}, 18, 17, rec, &produced), "beyond the bound"));
        CHECK(!kiss_encode_records({}, {}, {0}, 0, 0, rec, &produced) && rec.empty() && produced == 0);
    }
    std::printf("kiss host logic ok\n");
    return 0;
}
