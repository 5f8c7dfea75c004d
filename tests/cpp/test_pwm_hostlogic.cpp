// test_pwm_hostlogic.cpp — rustradio_amd/csrc/pwm_host.hpp without a device, built with the host sanitizers: every refusal of
// rr_pwm_decoder_create in validate()'s order and the limits of a handle, the refusals of a push, the plan of a push, the
// validation fed hostile device output, and the clamped copy-outs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rustradio_amd/csrc/pwm_host.hpp"

using namespace rr;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static std::string create(float hi, float lo, size_t s, size_t l, size_t tol, size_t fg, size_t rg, size_t fb, size_t mb, size_t md, size_t mr,
                          int flags = 0, size_t es = 4) {
    const char* e = pwm_check_create(hi, lo, s, l, tol, fg, rg, fb, mb, md, mr, flags, es);
    return e ? e : "";
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

int main() {
    // ---- create: validate() (src/pwm_decoder.rs:101-162), then the handle's own limits
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1) == "");
    CHECK(create(0.5f, 0.25f, 26, 80, 27, 110, 914, 25, 4096, 256, 3, RR_PWM_GAP_DELIMITER, 8) == "");
    CHECK(has(create(0.0f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1), "high threshold must be finite"));
    CHECK(has(create(INFINITY, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1), "high threshold"));
    CHECK(has(create(NAN, NAN, 0, 0, 0, 0, 0, 0, 0, 0, 0, 99, 3), "high threshold"));          // the first one said
    CHECK(has(create(0.5f, NAN, 2, 5, 1, 9, 20, 0, 16, 256, 1), "low threshold must be finite"));
    CHECK(has(create(0.5f, 0.0f, 2, 5, 1, 9, 20, 0, 16, 256, 1), "low threshold"));
    CHECK(has(create(0.5f, 0.75f, 2, 5, 1, 9, 20, 0, 16, 256, 1), "no greater than the high threshold"));
    CHECK(create(0.5f, 0.5f, 2, 5, 1, 9, 20, 0, 16, 256, 1) == "");
    CHECK(has(create(0.5f, 0.25f, 0, 5, 1, 9, 20, 0, 16, 256, 1), "short pulse width must be greater than zero"));
    CHECK(has(create(0.5f, 0.25f, 5, 5, 1, 9, 20, 0, 16, 256, 1), "long pulse width must be greater than the short"));
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 0, 20, 0, 16, 256, 1), "frame gap must be greater than zero"));
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 8, 0, 16, 256, 1), "reset gap must be at least as long"));
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 9, 0, 16, 256, 1) == "");
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 0, 256, 1), "maximum frame length must be greater than zero"));
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 17, 16, 256, 1), "fixed frame length exceeds the maximum"));
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 0, 1), "maximum distinct frames must be greater than zero"));
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 0), "minimum repeats must be greater than zero"));
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1, 4) == "unknown pwm decoder flags");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1, -1) == "unknown pwm decoder flags");
    CHECK(has(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 1, 0, 2), "Float (4) or Complex (8)"));
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16384, 256, 1) == "");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16385, 1, 1) == "pwm decoder: max_frame_bits beyond 16384");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 1025, 1) == "pwm decoder: max_distinct_frames beyond 1024");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 4096, 1024, 1) == "");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 4097, 1024, 1) == "pwm decoder: max_frame_bits x max_distinct_frames beyond 4194304");
    CHECK(create(0.5f, 0.25f, 2, ((size_t)1 << 62) + 1, 1, 9, 20, 0, 16, 256, 1) == "pwm decoder: width or gap beyond 2^62");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, ((size_t)1 << 62) + 1, 0, 16, 256, 1) == "pwm decoder: width or gap beyond 2^62");
    CHECK(create(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, (size_t)1 << 32) == "pwm decoder: min_repeats beyond 2^32 - 1");
    const PwmCfg c = pwm_cfg(0.5f, 0.25f, 2, 5, 1, 9, 20, 0, 16, 256, 3, RR_PWM_SHORT_IS_ZERO | RR_PWM_GAP_DELIMITER);
    CHECK(c.short_is_one == 0 && c.delimiter == 1 && c.min_repeats == 3 && c.frame_bits == 0 && c.max_bits == 16);
    // ---- push
    float x = 0;
    CHECK(pwm_check_push(&x, 1, false) == nullptr && pwm_check_push(nullptr, 0, false) == nullptr);
    CHECK(has(pwm_check_push(nullptr, 1, false), "null samples"));
    CHECK(has(pwm_check_push(&x, ((size_t)1 << 30) + 1, false), "more than 2^30"));
    CHECK(pwm_check_push(&x, (size_t)1 << 30, false) == nullptr);
    CHECK(has(pwm_check_push(&x, 1, true), "push after flush") && has(pwm_check_push(nullptr, 0, true), "push after flush"));
    // ---- the plan: everything from n and the settings
    const PwmPlan p1 = pwm_plan(1, 16, 4), pt = pwm_plan(PWM_T, 16, 4), pt1 = pwm_plan(PWM_T + 1, 16, 4), pf = pwm_plan(0, 16, 4);
    CHECK(p1.ntiles == 1 && p1.nthreads == PWM_B && p1.ecap == 1 && p1.frames == 4 + 2 && p1.arena == 64 + 16 + 2);
    CHECK(pt.ntiles == 1 && pt1.ntiles == 2 && pt1.nthreads == 2 * PWM_B && pt1.ecap == PWM_T + 1);
    CHECK(pf.ntiles == 0 && pf.frames == 4 && pf.arena == 64);
    const PwmPlan big = pwm_plan((size_t)1 << 30, 4096, 1024);
    CHECK(big.ntiles == ((size_t)1 << 30) / PWM_T && big.frames == 1024 + ((size_t)1 << 29) + 2);
    // ---- what the device wrote
    CHECK(pwm_check_counts(6, 82, p1) == nullptr && pwm_check_counts(7, 0, p1) != nullptr && pwm_check_counts(0, 83, p1) != nullptr);
    CHECK(pwm_check_counts(~0ull, ~0ull, p1) != nullptr);
    const PwmPlan p = pwm_plan(1000, 16, 4);
    auto rec = [](unsigned long long first, unsigned long long start, unsigned len, unsigned rep) {
        rr_pwm_frame r;
        r.first_sample = first; r.start = start; r.len = len; r.repeats = rep;
        return r;
    };
    std::vector<rr_pwm_frame> r = {rec(10, 0, 5, 3), rec(200, 5, 16, 4)};
    CHECK(pwm_validate(r, 21, p, 16, 3, 1000) == nullptr && r.size() == 2);
    struct Bad { std::vector<rr_pwm_frame> r; unsigned long long bits; const char* why; };
    const std::vector<Bad> bad = {
        {{rec(10, 0, 0, 3)}, 0, "length"}, {{rec(10, 0, 17, 3)}, 17, "length"}, {{rec(10, 1, 5, 3)}, 6, "outside the arena"},
        {{rec(10, 0, 5, 3), rec(20, 4, 5, 3)}, 10, "outside the arena"}, {{rec(10, 0, 5, 3)}, 4, "outside the arena"},
        {{rec(10, 0, 5, 2)}, 5, "min_repeats"}, {{rec(1000, 0, 5, 3)}, 5, "first sample"}, {{rec(10, 0, 5, 3)}, 6, "disagree"},
        {{rec(10, ~0ull, 5, 3)}, 5, "outside the arena"}, {{rec(10, 0, 5, 3)}, ~0ull, "beyond the bound"},
    };
    for (const Bad& b : bad) {
        std::vector<rr_pwm_frame> v = b.r;
        const char* e = pwm_validate(v, b.bits, p, 16, 3, 1000);
        CHECK(e && has(e, b.why) && v.empty());
    }
    std::vector<rr_pwm_frame> many(p.frames + 1, rec(1, 0, 1, 3));
    CHECK(pwm_validate(many, 1, p, 16, 3, 1000) != nullptr && many.empty());
    CHECK(pwm_validate_bits({0, 1, 1, 0}) == nullptr && pwm_validate_bits({0, 2}) != nullptr && pwm_validate_bits({}) == nullptr);
    // ---- the copy-outs
    std::vector<rr_pwm_frame> two = {rec(1, 0, 2, 3), rec(2, 2, 3, 3)};
    rr_pwm_frame out[2];
    std::memset(out, 0xff, sizeof out);
    size_t total = 99;
    pwm_copy_frames(two, nullptr, 0, &total);
    CHECK(total == 2);
    pwm_copy_frames(two, out, 1, &total);
    CHECK(total == 2 && out[0].first_sample == 1 && out[1].len == 0xffffffffu);
    unsigned char ob[4] = {9, 9, 9, 9};
    pwm_copy_bits({1, 0, 1}, ob, 2, &total);
    CHECK(total == 3 && ob[0] == 1 && ob[1] == 0 && ob[2] == 9);
    pwm_copy_bits({1, 0, 1}, nullptr, 0, &total);
    CHECK(total == 3);
    // ---- the sequential machine on the reference's first test (:731-754)
    {
        const PwmCfg k = pwm_cfg(0.5f, 0.25f, 2, 5, 1, 9, 20, 5, 16, 256, 3, RR_PWM_GAP_DELIMITER);
        std::vector<float> s(20, 0.0f);
        auto frame = [&](const char* bits) {
            for (const char* b = bits; *b; b++) { s.insert(s.end(), *b == '1' ? 2 : 5, 1.0f); s.insert(s.end(), *b == '1' ? 5 : 2, 0.0f); }
            s.insert(s.end(), 2, 1.0f);
            s.insert(s.end(), 9, 0.0f);
        };
        frame("11111");
        const size_t first = s.size();
        for (int i = 0; i < 3; i++) frame("10110");
        s.insert(s.end(), 20, 0.0f);
        PwmMachine m(k);
        std::vector<PwmHostFrame> got;
        CHECK(m.push(s.data(), s.size(), got) == 1 && got[0].repeats == 3 && got[0].first_sample == first &&
              got[0].bits == std::vector<unsigned char>({1, 0, 1, 1, 0}));
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("pwm host logic ok\n");
    return 0;
}
