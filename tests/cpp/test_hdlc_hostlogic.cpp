// The host-only logic of rr_hdlc_deframer_create / _push / _push_dev, rr_hdlc_frames, rr_hdlc_frame_bytes and rr_hdlc_stats
// (rustradio_amd/csrc/hdlc_host.hpp), driven without a device: the refusals, the carry bound, the bounds of a push, the validation
// of what a device wrote — fed hostile numbers, each of which must be refused with empty results — and the clamped copy-outs with
// guard elements behind `cap`; and many short-lived vectors, the handle churn of a test suite.  Built with
// -fsanitize=address,undefined and run by tests/test_hdlc_dev_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/hdlc_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static std::string str(const char* s) { return s ? s : ""; }
typedef unsigned long long u64;

static rr_hdlc_frame rec(u64 pos, u64 start, unsigned len, unsigned flags = 0) {
    rr_hdlc_frame r;
    r.pos = pos; r.start = start; r.len = len; r.flags = flags;
    return r;
}

int main() {
    using namespace rr;
    // create-time checks
    CHECK(hdlc_check_create(0, 0, 0) == nullptr && hdlc_check_create(10, 1500, 3) == nullptr && hdlc_check_create(70000, 65535, 1) == nullptr);
    CHECK(str(hdlc_check_create(1, 10, 4)) == "unknown hdlc deframer flags" && str(hdlc_check_create(1, 10, -1)) == "unknown hdlc deframer flags");
    CHECK(str(hdlc_check_create(1, 65536, 0)) == "hdlc deframer: max_size beyond 65535");
    CHECK(str(hdlc_check_create(1, ~(size_t)0, 0)) == "hdlc deframer: max_size beyond 65535");
    // push-time checks
    {
        const unsigned char one = 1;
        CHECK(hdlc_check_push(nullptr, 0) == nullptr && hdlc_check_push(&one, 1) == nullptr && hdlc_check_push(&one, (size_t)1 << 30) == nullptr);
        CHECK(str(hdlc_check_push(&one, ((size_t)1 << 30) + 1)) == "hdlc deframer: more than 2^30 bits in one push");
        CHECK(str(hdlc_check_push(nullptr, 1)) == "hdlc deframer: null bits");
    }
    // the carry bound: M + floor((M - 1) / 5) + 16, M = 8 max_size + 1
    CHECK(hdlc_carry_bits(0) == 1 + 0 + 16 && hdlc_carry_bits(1) == 9 + 1 + 16 && hdlc_carry_bits(3) == 25 + 4 + 16);
    CHECK(hdlc_carry_bits(1500) == 12001 + 2400 + 16 && hdlc_carry_bits(65535) == 524281 + 104856 + 16);
    for (size_t mx = 0; mx < 300; mx++) {           // R raw bits keep at least R - floor(R / 6): the bound is where that reaches M, not sooner
        const size_t M = 8 * mx + 1, R = (size_t)hdlc_reset_bits(mx);
        CHECK(R - R / 6 >= M && (R == 0 || (R - 1) - (R - 1) / 6 < M));
    }
    // the bounds of a push and the host's own count of the carried bits
    {
        HdlcBounds b = hdlc_bounds(8, 0);
        CHECK(b.nv == 8 && b.frames == 0 && b.arena == 1);
        b = hdlc_bounds(8, 1);
        CHECK(b.nv == 9 && b.frames == 1 && b.arena == 1);
        b = hdlc_bounds(45, 4096);
        CHECK(b.nv == 4141 && b.frames == 512 && b.arena == 517);
        b = hdlc_bounds(hdlc_carry_bits(65535), (size_t)1 << 30);
        CHECK(b.frames == (size_t)1 << 27 && b.arena == (hdlc_carry_bits(65535) + ((size_t)1 << 30)) / 8);
        size_t c = 8;
        c = hdlc_next_carry(c, 5, 3);
        CHECK(c == 13);
        c = hdlc_next_carry(c, 1000, 3);
        CHECK(c == hdlc_carry_bits(3));
        c = hdlc_next_carry(c, 0, 3);
        CHECK(c == hdlc_carry_bits(3));
    }
    // the plan of a push at the seams the kernels index by: tiles of HDLC_T = 4096 virtual bits, 64 words each and one more word;
    // a flag end every 7 bits and two more; blocks of HDLC_GB = 256 gaps
    {
        HdlcPlan p = hdlc_plan(8, 1, 50);
        CHECK(p.one.nv == 9 && p.ntiles == 1 && p.nwords == 65 && p.ecap == 3 && p.nblocks == 1 && p.one.frames == 1 && p.one.arena == 1);
        CHECK(p.carry_cap == hdlc_carry_bits(50));
        p = hdlc_plan(8, 4088, 50);
        CHECK(p.one.nv == 4096 && p.ntiles == 1);
        p = hdlc_plan(8, 4089, 50);
        CHECK(p.one.nv == 4097 && p.ntiles == 2 && p.nwords == 129);
        p = hdlc_plan(8, 1776, 50);
        CHECK(p.one.nv == 1784 && p.ecap == 256 && p.nblocks == 1);
        p = hdlc_plan(8, 1777, 50);
        CHECK(p.one.nv == 1785 && p.ecap == 257 && p.nblocks == 2);
        CHECK(p.carry_cap == hdlc_carry_bits(50) && hdlc_plan(45, 4096, 0).carry_cap == hdlc_carry_bits(0));
        const HdlcBounds b = hdlc_bounds(45, 4096);                 // `one` is hdlc_bounds of the same push
        p = hdlc_plan(45, 4096, 1500);
        CHECK(p.one.nv == b.nv && p.one.frames == b.frames && p.one.arena == b.arena);
    }
    // the validation
    const u64 zero[3] = {0, 0, 0};
    {
        const HdlcBounds b = hdlc_bounds(8, 800);                 // 100 frames, 101 arena bytes
        CHECK(hdlc_check_count(0, b) == nullptr && hdlc_check_count(100, b) == nullptr);
        CHECK(str(hdlc_check_count(101, b)) == "hdlc deframer: frame count beyond the bound");
        CHECK(str(hdlc_check_count(~0ull, b)) == "hdlc deframer: frame count beyond the bound");

        // a good push: sorted on the way
        std::vector<rr_hdlc_frame> r = {rec(1500, 60, 10, 1), rec(1015, 2, 0), rec(1799, 91, 10)};
        const u64 before[3] = {5, 6, 7}, after[3] = {8, 6, 8};
        CHECK(hdlc_validate(r, b, 10, 1000, 800, before, after) == nullptr);
        CHECK(r.size() == 3 && r[0].pos == 1015 && r[1].pos == 1500 && r[2].pos == 1799 && r[1].flags == 1);
        // ... and nothing at all
        std::vector<rr_hdlc_frame> none;
        CHECK(hdlc_validate(none, b, 10, 1000, 800, before, before) == nullptr && none.empty());

        struct Hostile { std::vector<rr_hdlc_frame> r; u64 after[3]; const char* why; };
        const std::vector<Hostile> hostile = {
            {std::vector<rr_hdlc_frame>(101, rec(1000, 0, 0)), {106, 6, 7}, "hdlc deframer: frame count beyond the bound"},
            {{rec(1100, 92, 10)}, {6, 6, 7}, "hdlc deframer: frame outside the arena"},
            {{rec(1100, 102, 0)}, {6, 6, 7}, "hdlc deframer: frame outside the arena"},
            {{rec(1100, ~0ull, 2)}, {6, 6, 7}, "hdlc deframer: frame outside the arena"},
            {{rec(1100, ~0ull - 1, 10)}, {6, 6, 7}, "hdlc deframer: frame outside the arena"},
            {{rec(1100, 0, 11)}, {6, 6, 7}, "hdlc deframer: frame longer than max_size"},
            {{rec(1100, 0, ~0u)}, {6, 6, 7}, "hdlc deframer: frame longer than max_size"},
            {{rec(1200, 30, 4), rec(1100, 10, 4), rec(1200, 50, 4)}, {8, 6, 7}, "hdlc deframer: two frames at one position"},
            {{rec(999, 0, 4)}, {6, 6, 7}, "hdlc deframer: frame position outside the push"},
            {{rec(1800, 0, 4)}, {6, 6, 7}, "hdlc deframer: frame position outside the push"},
            {{rec(~0ull, 0, 4)}, {6, 6, 7}, "hdlc deframer: frame position outside the push"},
            {{rec(1100, 0, 4, 2)}, {6, 6, 7}, "hdlc deframer: unknown record flags"},
            {{rec(1100, 0, 4)}, {4, 6, 7}, "hdlc deframer: a counter ran backwards"},
            {{rec(1100, 0, 4)}, {6, 5, 7}, "hdlc deframer: a counter ran backwards"},
            {{rec(1100, 0, 4)}, {6, 6, 0}, "hdlc deframer: a counter ran backwards"},
            {{rec(1100, 0, 4)}, {7, 6, 7}, "hdlc deframer: decoded counter and frame count disagree"},
            {{}, {6, 6, 7}, "hdlc deframer: decoded counter and frame count disagree"},
        };
        for (const Hostile& h : hostile) {
            std::vector<rr_hdlc_frame> got = h.r;
            const char* e = hdlc_validate(got, b, 10, 1000, 800, before, h.after);
            if (str(e) != h.why) std::printf("hostile case: got \"%s\", want \"%s\"\n", str(e).c_str(), h.why);
            CHECK(str(e) == h.why && got.empty());
        }
        // max_size 0: only empty frames pass
        std::vector<rr_hdlc_frame> e0 = {rec(1100, 3, 0)}, e1 = {rec(1100, 3, 1)};
        const u64 one[3] = {1, 0, 0};
        CHECK(hdlc_validate(e0, b, 0, 1000, 800, zero, one) == nullptr && e0.size() == 1);
        CHECK(hdlc_validate(e1, b, 0, 1000, 800, zero, one) != nullptr && e1.empty());
        // an empty push has room for nothing
        const HdlcBounds nothing = hdlc_bounds(8, 0);
        std::vector<rr_hdlc_frame> x = {rec(1000, 0, 0)};
        CHECK(hdlc_validate(x, nothing, 10, 1000, 0, zero, one) != nullptr && x.empty());
    }
    // the copy-outs at cap 0, 1, total - 1, total, total + 1 and NULL, with guard elements behind cap
    {
        std::vector<rr_hdlc_frame> r;
        for (unsigned i = 0; i < 5; i++) r.push_back(rec(100 + i, 8 * i, i));
        const size_t caps[] = {0, 1, 4, 5, 6};
        for (size_t cap : caps) {
            std::vector<rr_hdlc_frame> out(cap + 2, rec(~0ull, ~0ull, ~0u, ~0u));
            size_t total = 99;
            hdlc_copy_frames(r, out.data(), cap, &total);
            CHECK(total == 5);
            for (size_t i = 0; i < out.size(); i++) {
                if (i < cap && i < 5) CHECK(out[i].pos == 100 + i && out[i].len == i);
                else CHECK(out[i].pos == ~0ull && out[i].flags == ~0u);
            }
        }
        size_t total = 99;
        hdlc_copy_frames(r, nullptr, 0, &total);
        CHECK(total == 5);
        hdlc_copy_frames(std::vector<rr_hdlc_frame>(), nullptr, 0, &total);
        CHECK(total == 0);

        std::vector<unsigned char> a = {1, 2, 3, 4, 5};
        for (size_t cap : caps) {
            std::vector<unsigned char> out(cap + 2, 0xee);
            size_t tb = 99;
            hdlc_copy_bytes(a, out.data(), cap, &tb);
            CHECK(tb == 5);
            for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == (i < cap && i < 5 ? i + 1 : 0xee));
        }
        hdlc_copy_bytes(a, nullptr, 0, &total);
        CHECK(total == 5);
        hdlc_copy_bytes(std::vector<unsigned char>(), nullptr, 0, &total);
        CHECK(total == 0);
    }
    // churn: what a suite of short pushes does to the heap
    for (int it = 0; it < 20000; it++) {
        const size_t n = 1 + (size_t)(it * 7919) % 5000;
        const HdlcBounds b = hdlc_bounds(hdlc_carry_bits((size_t)it % 12), n);
        const size_t k = (size_t)it % (b.frames + 1);
        std::vector<rr_hdlc_frame> r;
        for (size_t i = 0; i < k; i++) r.push_back(rec(50 + 8 * (k - 1 - i), i % (b.arena + 1), 0));
        const u64 after[3] = {k, 0, 0};
        CHECK(hdlc_validate(r, b, (size_t)it % 12, 50, n, zero, after) == nullptr && r.size() == k);
        std::vector<rr_hdlc_frame> out(k / 2 + 1);
        size_t total = 0;
        hdlc_copy_frames(r, out.data(), k / 2, &total);
        CHECK(total == k);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("hdlc host logic ok\n");
    return 0;
}
