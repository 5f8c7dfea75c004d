// The host-only logic of rr_il2p_receiver_create / _push / _push_dev / _headers / _stats / _consumed
// (rustradio_amd/csrc/il2p_host.hpp), driven without a device: every refusal, the bounds of a push, the clamping of the stream
// positions, the validation of what a device wrote — fed hostile numbers, each of which must be refused with empty results — the
// ordering, and the clamped copy-outs with guard elements behind `cap`.  Built with -fsanitize=address,undefined and run by
// tests/test_il2p_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/il2p_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static std::string str(const char* s) { return s ? s : ""; }
typedef unsigned long long u64;

static rr_il2p_header rec(unsigned stream, u64 pos) {
    rr_il2p_header r;
    std::memset(&r, 0, sizeof r);
    r.pos = pos; r.stream = stream;
    return r;
}

int main() {
    using namespace rr;
    // ---- create-time refusals ----------------------------------------------------------------------------------------------------------
    CHECK(il2p_check_create(1, 0) == nullptr && il2p_check_create(4096, RR_BITS_INVERT) == nullptr);
    CHECK(str(il2p_check_create(0, 0)) == "nstreams out of range");
    CHECK(str(il2p_check_create(4097, 0)) == "nstreams out of range");
    CHECK(str(il2p_check_create(0, 8)) == "nstreams out of range");               // nstreams first
    CHECK(str(il2p_check_create(3, RR_BITS_NRZI)) == "il2p receiver: unknown bit flags");
    CHECK(str(il2p_check_create(3, RR_BITS_INVERT | RR_BITS_DESCRAMBLE)) == "il2p receiver: unknown bit flags");
    CHECK(str(il2p_check_create(3, -1)) == "il2p receiver: unknown bit flags");
    CHECK(il2p_clamp_allowed(0) == 0 && il2p_clamp_allowed(3) == 3 && il2p_clamp_allowed(24) == 24 && il2p_clamp_allowed(25) == 24 &&
          il2p_clamp_allowed(~(size_t)0) == 24);
    // ---- push-time refusals ------------------------------------------------------------------------------------------------------------
    {
        const float one = 1.0f;
        CHECK(il2p_check_push(5, nullptr, 0, 0) == nullptr && il2p_check_push(5, &one, 10, 10) == nullptr && il2p_check_push(5, &one, 11, 10) == nullptr);
        CHECK(str(il2p_check_push(5, &one, 9, 10)) == "il2p receiver: stride shorter than n_cap");
        CHECK(str(il2p_check_push(5, nullptr, 10, 10)) == "il2p receiver: null symbols");
        CHECK(il2p_check_push(5, nullptr, 10, 0) == nullptr);                       // n_cap == 0: nothing is read
        CHECK(il2p_check_push(4096, &one, (size_t)1 << 18, (size_t)1 << 18) == nullptr);
        CHECK(str(il2p_check_push(4096, &one, ((size_t)1 << 18) + 1, ((size_t)1 << 18) + 1)) == "il2p receiver: more than 2^30 symbols in one push");
        CHECK(il2p_check_push(1, &one, (size_t)1 << 30, (size_t)1 << 30) == nullptr);
        CHECK(str(il2p_check_push(1, &one, ((size_t)1 << 30) + 1, ((size_t)1 << 30) + 1)) == "il2p receiver: more than 2^30 symbols in one push");
        CHECK(str(il2p_check_push(3, &one, ~(size_t)0, ~(size_t)0)) == "il2p receiver: more than 2^30 symbols in one push");
    }
    // ---- the bounds ------------------------------------------------------------------------------------------------------------------------
    {
        CHECK(il2p_max_headers(0) == 0 && il2p_max_headers(1) == 1 && il2p_max_headers(2) == 2 && il2p_max_headers(121) == 2 &&
              il2p_max_headers(122) == 2 && il2p_max_headers(123) == 3 && il2p_max_headers(1210) == 11);
        // what a push can really emit: tags at -120, 1, 122, ... with the last at most at n - 121
        for (size_t n = 1; n < 2000; n++) CHECK((n - 1) / 121 + 1 <= il2p_max_headers(n));
        const Il2pBounds b = il2p_bounds(3, 4097);
        CHECK(b.nstreams == 3 && b.n_cap == 4097 && b.tiles == 2 && b.words == 3 + 128 + 1 && b.per_stream == 35 && b.headers == 105);
        const Il2pBounds z = il2p_bounds(7, 0);
        CHECK(z.tiles == 0 && z.headers == 0 && z.words == 4);
        CHECK(il2p_check_count(105, b) == nullptr && str(il2p_check_count(106, b)) == "il2p receiver: header count beyond the bound");
        CHECK(str(il2p_check_count(~0ull, b)) == "il2p receiver: header count beyond the bound");
        const Il2pBounds big = il2p_bounds(1, (size_t)1 << 30);
        CHECK(big.tiles == (size_t)1 << 18 && big.headers == ((((size_t)1 << 30) + 119) / 121 + 1));
    }
    // ---- the clamping of positions ---------------------------------------------------------------------------------------------------------
    {
        const u64 before[3] = {100, 0, 5}, after[3] = {100, 4097, 5000000};
        std::vector<size_t> moved;
        CHECK(il2p_clamp_consumed(before, after, 3, 4097, moved) == nullptr && moved.size() == 3 && moved[0] == 0 && moved[1] == 4097 && moved[2] == 4097);
        const u64 back[3] = {99, 0, 5};
        CHECK(str(il2p_clamp_consumed(before, back, 3, 4097, moved)) == "il2p receiver: a stream position ran backwards");
        CHECK(moved.size() == 3 && moved[0] == 0 && moved[1] == 0 && moved[2] == 0);
    }
    // ---- the validation ----------------------------------------------------------------------------------------------------------------------
    {
        const Il2pBounds b = il2p_bounds(3, 1000);
        const u64 pos0[3] = {5000, 0, 700};
        const size_t moved[3] = {1000, 1000, 300};
        // fine, and sorted by (stream, pos): a header that began in front of the push, one that ends on its last symbol
        std::vector<rr_il2p_header> ok = {rec(2, 700), rec(0, 5879), rec(1, 23), rec(0, 4880), rec(1, 144), rec(0, 5001)};
        CHECK(il2p_validate(ok, b, pos0, moved) == nullptr && ok.size() == 6);
        CHECK(ok[0].stream == 0 && ok[0].pos == 4880 && ok[1].pos == 5001 && ok[2].pos == 5879 && ok[3].stream == 1 && ok[3].pos == 23 &&
              ok[4].pos == 144 && ok[5].stream == 2);
        std::vector<rr_il2p_header> none;
        CHECK(il2p_validate(none, b, pos0, moved) == nullptr && none.empty());
        // hostile
        std::vector<rr_il2p_header> r = {rec(3, 100)};                             // stream == nstreams
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: no such stream" && r.empty());
        r = {rec(~0u, 100)};
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: no such stream" && r.empty());
        r = {rec(0, 5880)};                                                        // its 120th bit lies behind the push
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header position outside the push" && r.empty());
        r = {rec(0, 4879)};                                                        // ... in front of it
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header position outside the push" && r.empty());
        r = {rec(2, 880)};                                                         // beyond what the stream took (300 of 1000)
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header position outside the push" && r.empty());
        r = {rec(1, 22)};                                                          // no tag before 24 bits were seen
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header position outside the stream" && r.empty());
        r = {rec(1, ~0ull - 5)};                                                   // pos + 120 wraps
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header position outside the stream" && r.empty());
        r = {rec(1, 500), rec(0, 5100), rec(1, 620)};                              // two headers of one stream closer than 121
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: two headers closer than 121" && r.empty());
        r = {rec(1, 500), rec(1, 500)};
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: two headers closer than 121" && r.empty());
        r = {rec(1, 500), rec(0, 5500), rec(1, 621)};                              // exactly 121 apart, and the same pos in two streams
        CHECK(il2p_validate(r, b, pos0, moved) == nullptr && r.size() == 3);
        r.assign(b.headers + 1, rec(1, 500));                                      // a count above the list
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header count beyond the bound" && r.empty());
        r = {rec(1, 500)};
        r[0].pid = 16;
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header field out of range" && r.empty());
        r = {rec(1, 500)};
        r[0].diffs = 25;
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header field out of range" && r.empty());
        r = {rec(1, 500)};
        r[0].payload_size = 1024;
        CHECK(str(il2p_validate(r, b, pos0, moved)) == "il2p receiver: header field out of range" && r.empty());
    }
    // ---- the copy-outs: nothing behind cap is written -------------------------------------------------------------------------------------
    {
        std::vector<rr_il2p_header> h = {rec(0, 100), rec(0, 300), rec(1, 50)};
        std::vector<rr_il2p_header> out(2, rec(9, 9));
        size_t total = 99;
        il2p_copy_headers(h, out.data(), 1, &total);
        CHECK(total == 3 && out[0].pos == 100 && out[1].stream == 9);
        il2p_copy_headers(h, nullptr, 0, &total);
        CHECK(total == 3);
        il2p_copy_headers({}, out.data(), 2, &total);
        CHECK(total == 0 && out[0].pos == 100);
        const std::vector<u64> v = {1, 2, 3, 4, 5, 6};
        u64 o[3] = {77, 77, 77};
        il2p_copy_u64(v, 1, 2, o, 2, &total);
        CHECK(total == 3 && o[0] == 2 && o[1] == 4 && o[2] == 77);
        il2p_copy_u64(v, 0, 2, nullptr, 3, &total);
        CHECK(total == 3);
        il2p_copy_u64(v, 0, 1, o, 3, &total);
        CHECK(total == 6 && o[0] == 1 && o[2] == 3);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("il2p host logic ok\n");
    return 0;
}
