// The host-only logic of rr_hdlc_receiver_create / _push / _push_dev / _frames / _frame_bytes / _stats / _consumed
// (rustradio_amd/csrc/hdlcrx_host.hpp), driven without a device: every refusal, the bounds of a push, the clamping of the stream
// positions, the validation of what a device wrote — fed hostile numbers, each of which must be refused with empty results — and
// the clamped copy-outs with guard elements behind `cap`.  Built with -fsanitize=address,undefined and run by
// tests/test_hdlcrx_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/hdlcrx_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static std::string str(const char* s) { return s ? s : ""; }
typedef unsigned long long u64;

static rr_hdlc_stream_frame rec(unsigned stream, u64 pos, u64 start, unsigned len, unsigned flags = 0, unsigned reserved = 0) {
    rr_hdlc_stream_frame r;
    r.pos = pos; r.start = start; r.len = len; r.flags = flags; r.stream = stream; r.reserved = reserved;
    return r;
}

int main() {
    using namespace rr;
    // ---- create-time refusals: nstreams first, then the bit decoder's, then the deframer's -------------------------------------------
    CHECK(hdlcrx_check_create(1, 0, 0, 0, 0, 0, 0) == nullptr && hdlcrx_check_create(4096, 7, 0, 16, 10, 1500, 3) == nullptr);
    CHECK(str(hdlcrx_check_create(0, 0, 0, 0, 1, 10, 0)) == "nstreams out of range");
    CHECK(str(hdlcrx_check_create(4097, 0, 0, 0, 1, 10, 0)) == "nstreams out of range");
    CHECK(str(hdlcrx_check_create(0, 8, 0, 0, 1, 10, 4)) == "nstreams out of range");
    CHECK(str(hdlcrx_check_create(3, 8, 0, 0, 1, 10, 0)) == "unknown bit decoder flags");
    CHECK(str(hdlcrx_check_create(3, -1, 0, 0, 1, 10, 0)) == "unknown bit decoder flags");
    CHECK(str(hdlcrx_check_create(3, 4, 0, 64, 1, 10, 0)) == "descrambler length out of range");
    CHECK(hdlcrx_check_create(3, 3, 0, 64, 1, 10, 0) == nullptr);                  // no descrambler: its parameters are not looked at
    CHECK(str(hdlcrx_check_create(3, 4, 1ull << 17, 16, 1, 10, 0)) == "seed wider than the register");
    CHECK(hdlcrx_check_create(3, 4, 1ull << 16, 16, 1, 10, 0) == nullptr && hdlcrx_check_create(3, 4, ~0ull, 63, 1, 10, 0) == nullptr);
    CHECK(str(hdlcrx_check_create(3, 4, 0, 16, 1, 10, 4)) == "unknown hdlc deframer flags");
    CHECK(str(hdlcrx_check_create(3, 4, 0, 16, 1, 65536, 0)) == "hdlc deframer: max_size beyond 65535");
    CHECK(str(hdlcrx_check_create(3, 8, 0, 16, 1, 65536, 0)) == "unknown bit decoder flags");
    // ---- push-time refusals ------------------------------------------------------------------------------------------------------------
    {
        const float one = 1.0f;
        CHECK(hdlcrx_check_push(5, nullptr, 0, 0) == nullptr && hdlcrx_check_push(5, &one, 10, 10) == nullptr && hdlcrx_check_push(5, &one, 11, 10) == nullptr);
        CHECK(str(hdlcrx_check_push(5, &one, 9, 10)) == "hdlc receiver: stride shorter than n_cap");
        CHECK(str(hdlcrx_check_push(5, nullptr, 10, 10)) == "hdlc receiver: null symbols");
        CHECK(hdlcrx_check_push(5, nullptr, 10, 0) == nullptr);                     // n_cap == 0: nothing is read
        CHECK(hdlcrx_check_push(4096, &one, (size_t)1 << 18, (size_t)1 << 18) == nullptr);
        CHECK(str(hdlcrx_check_push(4096, &one, ((size_t)1 << 18) + 1, ((size_t)1 << 18) + 1)) == "hdlc receiver: more than 2^30 symbols in one push");
        CHECK(hdlcrx_check_push(1, &one, (size_t)1 << 30, (size_t)1 << 30) == nullptr);
        CHECK(str(hdlcrx_check_push(1, &one, ((size_t)1 << 30) + 1, ((size_t)1 << 30) + 1)) == "hdlc receiver: more than 2^30 symbols in one push");
        CHECK(str(hdlcrx_check_push(3, &one, ~(size_t)0, ~(size_t)0)) == "hdlc receiver: more than 2^30 symbols in one push");
    }
    // ---- the bounds: one number serves all streams ----------------------------------------------------------------------------------------
    {
        const HdlcRxBounds b = hdlcrx_bounds(3, 45, 4096);
        CHECK(b.one.nv == 4141 && b.one.frames == 512 && b.one.arena == 517 && b.frames == 1536 && b.arena == 1551 && b.nstreams == 3);
        CHECK(hdlcrx_check_count(1536, b) == nullptr && str(hdlcrx_check_count(1537, b)) == "hdlc receiver: frame count beyond the bound");
        CHECK(str(hdlcrx_check_count(~0ull, b)) == "hdlc receiver: frame count beyond the bound");
        // one stream's share is the plan's of the same push (hdlc_plan sizes the workspace, these bounds the read-back)
        const size_t ns[] = {1, 4088, 4089, 1776, 1777, 1u << 20};
        for (size_t n : ns)
            for (size_t mx : {(size_t)0, (size_t)50, (size_t)65535}) {
                const HdlcBounds one = hdlcrx_bounds(3, 8, n).one, p = hdlc_plan(8, n, mx).one;
                CHECK(one.nv == p.nv && one.frames == p.frames && one.arena == p.arena);
            }
        size_t c = 8;
        c = hdlc_next_carry(c, 100, 40);
        CHECK(c == 108);
        c = hdlc_next_carry(c, 4096, 40);
        CHECK(c == hdlc_carry_bits(40) && c == 321 + 64 + 16);
    }
    // ---- counts and positions are clamped -------------------------------------------------------------------------------------------------
    {
        const u64 before[3] = {100, 0, ~0ull - 5}, after[3] = {100, 800, ~0ull};
        std::vector<size_t> moved;
        CHECK(hdlcrx_clamp_consumed(before, after, 3, 800, moved) == nullptr && moved == (std::vector<size_t>{0, 800, 5}));
        const u64 beyond[3] = {100 + 801, 1ull << 40, ~0ull};                       // counts beyond n_cap: clamped before anybody sees them
        CHECK(hdlcrx_clamp_consumed(before, beyond, 3, 800, moved) == nullptr && moved == (std::vector<size_t>{800, 800, 5}));
        const u64 back[3] = {99, 800, ~0ull};
        CHECK(str(hdlcrx_clamp_consumed(before, back, 3, 800, moved)) == "hdlc receiver: a stream position ran backwards");
        CHECK(moved == (std::vector<size_t>{0, 0, 0}));
    }
    // ---- the validation ---------------------------------------------------------------------------------------------------------------------
    {
        const HdlcRxBounds b = hdlcrx_bounds(3, 8, 800);                             // per stream 100 frames and 101 arena bytes
        CHECK(b.one.arena == 101 && b.one.frames == 100);
        const u64 pos0[3] = {1000, 0, 5000};
        const size_t moved[3] = {800, 800, 0};
        const u64 z[9] = {7, 1, 1, 0, 0, 0, 3, 3, 3};
        auto after = [&](u64 d0, u64 d1, u64 d2) { return std::vector<u64>{7 + d0, 1, 1, 0 + d1, 0, 0, 3 + d2, 3, 3}; };
        auto run = [&](std::vector<rr_hdlc_stream_frame> r, const std::vector<u64>& a, std::vector<rr_hdlc_stream_frame>* out = nullptr) {
            const char* e = hdlcrx_validate(r, b, 40, pos0, moved, z, a.data());
            if (e) CHECK(r.empty());
            if (out) *out = r;
            return str(e);
        };
        std::vector<rr_hdlc_stream_frame> out;
        // fine, and sorted by (stream, pos); the same pos in two streams is legal
        CHECK(run({rec(1, 500, 101 + 50, 10), rec(0, 1500, 60, 40, 1), rec(1, 20, 101, 0), rec(0, 1020, 0, 3)}, after(2, 2, 0), &out) == "");
        CHECK(out.size() == 4 && out[0].stream == 0 && out[0].pos == 1020 && out[1].pos == 1500 && out[2].stream == 1 && out[2].pos == 20 && out[3].pos == 500);
        CHECK(run({rec(0, 1020, 0, 3), rec(1, 1020 - 1000, 101, 3)}, after(1, 1, 0)) == "");
        {                                                                            // the very same pos in two streams
            const u64 p0[3] = {0, 0, 0}, s0[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, s1[9] = {1, 0, 0, 1, 0, 0, 0, 0, 0};
            const size_t mv[3] = {800, 800, 800};
            std::vector<rr_hdlc_stream_frame> r = {rec(1, 100, 101, 3), rec(0, 100, 0, 3)};
            CHECK(hdlcrx_validate(r, b, 40, p0, mv, s0, s1) == nullptr && r.size() == 2 && r[0].stream == 0 && r[1].stream == 1);
        }
        CHECK(run({rec(0, 1500, 0, 3), rec(1, 500, 101, 3), rec(1, 799, 202 - 3, 3)}, after(1, 2, 0)) == "");
        CHECK(run({}, after(0, 0, 0)) == "");
        // stream == nstreams, and beyond
        CHECK(run({rec(3, 10, 303, 1)}, after(0, 0, 1)) == "hdlc receiver: no such stream");
        CHECK(run({rec(~0u, 10, 0, 1)}, after(1, 0, 0)) == "hdlc receiver: no such stream");
        // a record of another stream's arena region
        CHECK(run({rec(1, 500, 50, 10)}, after(0, 1, 0)) == "hdlc receiver: frame outside its stream's arena");
        CHECK(run({rec(0, 1500, 101, 1)}, after(1, 0, 0)) == "hdlc receiver: frame outside its stream's arena");
        CHECK(run({rec(0, 1500, 95, 7)}, after(1, 0, 0)) == "hdlc receiver: frame outside its stream's arena");        // runs over into stream 1's
        CHECK(run({rec(0, 1500, 101, 0)}, after(1, 0, 0)) == "");                                                        // (empty, at its region's end)
        CHECK(run({rec(1, 500, 202, 1)}, after(0, 1, 0)) == "hdlc receiver: frame outside its stream's arena");
        CHECK(run({rec(1, 500, ~0ull, 1)}, after(0, 1, 0)) == "hdlc receiver: frame outside its stream's arena");
        CHECK(run({rec(0, 1500, 0, 41)}, after(1, 0, 0)) == "hdlc receiver: frame longer than max_size");
        CHECK(run({rec(0, 1500, 0, ~0u)}, after(1, 0, 0)) == "hdlc receiver: frame longer than max_size");
        // positions: inside that stream's own symbols of this push
        CHECK(run({rec(0, 999, 0, 3)}, after(1, 0, 0)) == "hdlc receiver: frame position outside the push");
        CHECK(run({rec(0, 1800, 0, 3)}, after(1, 0, 0)) == "hdlc receiver: frame position outside the push");
        CHECK(run({rec(1, 1020, 101, 3)}, after(0, 1, 0)) == "hdlc receiver: frame position outside the push");        // (fine in stream 0)
        CHECK(run({rec(2, 5000, 202, 3)}, after(0, 0, 1)) == "hdlc receiver: frame position outside the push");        // a stream that got no symbols
        // flags
        CHECK(run({rec(0, 1500, 0, 3, 2)}, after(1, 0, 0)) == "hdlc receiver: unknown record flags");
        CHECK(run({rec(0, 1500, 0, 3, 0, 1)}, after(1, 0, 0)) == "hdlc receiver: unknown record flags");
        // a duplicate pos within a stream
        CHECK(run({rec(1, 500, 101, 3), rec(0, 1500, 0, 3), rec(1, 500, 110, 3)}, after(1, 2, 0)) == "hdlc receiver: two frames at one position");
        // the counters
        CHECK(run({rec(0, 1500, 0, 3)}, {8, 0, 1, 0, 0, 0, 3, 3, 3}) == "hdlc receiver: a counter ran backwards");
        CHECK(run({}, {7, 1, 1, 0, 0, 0, 3, 3, 2}) == "hdlc receiver: a counter ran backwards");
        CHECK(run({}, {6, 1, 1, 1, 0, 0, 3, 3, 3}) == "hdlc receiver: a counter ran backwards");                       // (the sum would have hidden it)
        CHECK(run({rec(0, 1500, 0, 3)}, after(0, 0, 0)) == "hdlc receiver: decoded counters and frame count disagree");
        CHECK(run({rec(0, 1500, 0, 3)}, after(1, 1, 0)) == "hdlc receiver: decoded counters and frame count disagree");
        CHECK(run({rec(0, 1500, 0, 3)}, after(0, 1, 0)) == "");      // only the sum is held against the list: which stream decoded is the counters' word
        // more records than the bound
        std::vector<rr_hdlc_stream_frame> many(301, rec(0, 1500, 0, 3));
        CHECK(run(many, after(301, 0, 0)) == "hdlc receiver: frame count beyond the bound");
    }
    // ---- the copy-outs ------------------------------------------------------------------------------------------------------------------------
    {
        std::vector<rr_hdlc_stream_frame> r = {rec(0, 1, 2, 3), rec(1, 4, 5, 6), rec(2, 7, 8, 9)};
        std::vector<rr_hdlc_stream_frame> out(2, rec(9, 9, 9, 9));                  // (exactly cap long: the sanitizer sees a write behind it)
        size_t total = 99;
        hdlcrx_copy_frames(r, nullptr, 0, &total);
        CHECK(total == 3);
        hdlcrx_copy_frames(r, out.data(), 2, &total);
        CHECK(total == 3 && out[0].pos == 1 && out[1].stream == 1 && out[1].pos == 4);
        std::vector<rr_hdlc_stream_frame> big(5, rec(9, 9, 9, 9));
        hdlcrx_copy_frames(r, big.data(), 5, &total);
        CHECK(total == 3 && big[2].pos == 7 && big[3].pos == 9);
        const std::vector<u64> s = {1, 2, 3, 4, 5, 6};
        std::vector<u64> o(1, 77);
        hdlcrx_copy_u64(s, 1, 3, o.data(), 1, &total);
        CHECK(total == 2 && o[0] == 2);
        hdlcrx_copy_u64(s, 2, 3, nullptr, 0, &total);
        CHECK(total == 2);
        hdlcrx_copy_u64(s, 0, 3, nullptr, 5, &total);                                // an array the caller does not want
        CHECK(total == 2);
        std::vector<u64> o3(3, 77);
        hdlcrx_copy_u64(s, 0, 1, o3.data(), 3, &total);
        CHECK(total == 6 && o3[2] == 3);
    }
    for (int i = 0; i < 2000; i++) {                 // handle churn: many short-lived vectors through the validation
        std::vector<rr_hdlc_stream_frame> r((size_t)(i % 7), rec(0, 0, 0, 0));
        for (size_t k = 0; k < r.size(); k++) r[k] = rec((unsigned)(k % 2), 10 + k, (k % 2) * 13, 2);
        const HdlcRxBounds b = hdlcrx_bounds(2, 8, 96);
        const u64 p0[2] = {0, 0}, s0[6] = {0, 0, 0, 0, 0, 0};
        const size_t mv[2] = {96, 96};
        const u64 s1[6] = {(r.size() + 1) / 2, 0, 0, r.size() / 2, 0, 0};
        CHECK(hdlcrx_validate(r, b, 10, p0, mv, s0, s1) == nullptr);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("hdlcrx host logic ok\n");
    return 0;
}
