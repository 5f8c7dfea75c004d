// The host-only logic of rr_delay and rr_burst_saver (rustradio_amd/csrc/saver_host.hpp), driven without a device: the refusals,
// one work() of Delay against the reference's loop written out, the history plan against a simulation of many pushes shorter
// than the delay, and the launch count.  Built with -fsanitize=address,undefined and run by tests/test_saver_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/saver_host.hpp"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

// delay.rs:64-110 as written (no skip): one decision per turn of the loop
static rr::DelayStep loop_step(size_t& remaining, size_t in_len, size_t out_cap) {
    rr::DelayStep d{0, 0, 0};
    size_t in_left = in_len, room = out_cap;
    for (;;) {
        if (room == 0) { d.status = RR_WAIT_DST; return d; }
        if (remaining > 0) {
            const size_t n = std::min(remaining, room);
            d.zeros += n; room -= n; remaining -= n;
            continue;
        }
        if (in_left == 0) { d.status = RR_WAIT_SRC; return d; }
        const size_t n = std::min(in_left, room);
        d.copied += n; in_left -= n; room -= n;
    }
}

int main() {
    using namespace rr;
    // the refusals, each with its sentence
    CHECK(delay_check(0, 1) == nullptr && delay_check(DELAY_MAX, 4) == nullptr && delay_check(7, 8) == nullptr);
    for (size_t es : {(size_t)0, (size_t)2, (size_t)3, (size_t)16}) CHECK(std::string(delay_check(1, es)) == "unsupported element size");
    CHECK(std::string(delay_check(DELAY_MAX + 1, 4)) == "delay: more than 1,024,000 samples");
    CHECK(std::string(delay_check(DELAY_MAX + 1, 3)) == "unsupported element size");
    CHECK(saver_check(0.0f, 0, 0) == nullptr && saver_check(1.0f, DELAY_MAX, 512000) == nullptr);
    CHECK(std::string(saver_check(-0.5f, 1, 1)) == "alpha out of range");
    CHECK(std::string(saver_check(std::strtof("nan", nullptr), 1, 1)) == "alpha out of range");
    CHECK(std::string(saver_check(0.5f, 1, 512001)) == "max_size beyond 512000 samples");
    CHECK(std::string(saver_check(0.5f, DELAY_MAX + 1, 10)) == "delay: more than 1,024,000 samples");
    int x = 0;
    CHECK(saver_push_check(nullptr, 0) == nullptr && saver_push_check(&x, SAVER_MAX_WINDOW) == nullptr);
    CHECK(std::string(saver_push_check(&x, SAVER_MAX_WINDOW + 1)) == "window longer than 1024000 samples");
    CHECK(std::string(saver_push_check(nullptr, 1)) == "null argument");

    // delay_step is the loop, for every small case
    for (size_t rem = 0; rem <= 6; rem++)
        for (size_t in_len = 0; in_len <= 6; in_len++)
            for (size_t cap = 0; cap <= 8; cap++) {
                size_t r0 = rem, r1 = rem;
                const DelayStep a = delay_step(r0, in_len, cap), b = loop_step(r1, in_len, cap);
                CHECK(a.zeros == b.zeros && a.copied == b.copied && a.status == b.status && r0 == r1);
                CHECK(a.zeros + a.copied <= cap && a.copied <= in_len);
            }

    // the history plan: the delayed stream and the next history, pushes shorter than the delay and many of them in a row,
    // against the whole-stream statement d[p] = p < delay ? 0 : x[p - delay].  The vectors are exactly sized: an index the
    // plan gets wrong is the sanitizer's.
    for (size_t delay : {(size_t)0, (size_t)1, (size_t)5, (size_t)30}) {
        std::vector<int> hist(delay, 0), stream;
        size_t seed = 1;
        for (int push = 0; push < 60; push++) {
            seed = seed * 1103515245 + 12345;
            const size_t n = push < 40 ? (seed >> 16) % 4 : (seed >> 16) % 50;        // 40 pushes of 0..3 samples first
            std::vector<int> xs(n), out(n), next(delay);
            for (size_t i = 0; i < n; i++) xs[i] = (int)(stream.size() + i + 1);
            const SaverPlan pl = saver_plan(n, delay);
            CHECK(pl.from_hist == std::min(n, delay) && pl.shifted + pl.from_hist == delay);
            if (n) {
                for (size_t i = 0; i < n; i++) out[i] = i < pl.from_hist ? hist.at(i) : xs.at(i - delay);
                for (size_t j = 0; j < delay; j++) next[j] = j < pl.shifted ? hist.at(j + n) : xs.at(j + n - delay);
                hist.swap(next);
            }
            for (size_t i = 0; i < n; i++) {
                const size_t p = stream.size() + i;
                CHECK(out[i] == (p < delay ? 0 : (int)(p - delay + 1)));
            }
            stream.insert(stream.end(), xs.begin(), xs.end());
        }
    }

    // launches: the envelope's 1 or 3, the copy, StreamToPdu's 5 + ceil(log2(n / 2 + 1))
    CHECK(saver_launches(0, 2048) == 0);
    CHECK(saver_launches(1, 2048) == 1 + 1 + 5 + 0);
    CHECK(saver_launches(2, 2048) == 1 + 1 + 5 + 1);
    CHECK(saver_launches(2048, 2048) == 1 + 1 + 5 + 11);
    CHECK(saver_launches(2049, 2048) == 3 + 1 + 5 + 11);
    CHECK(saver_launches(4096, 2048) == 3 + 1 + 5 + 12);

    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("saver host logic ok\n");
    return 0;
}
