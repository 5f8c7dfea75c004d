// emu_pwm.cpp — rustradio_amd/csrc/pwm_core.hpp run tile by tile and thread by thread on the CPU, in the order of the kernels of
// kernels_pwm.hip (classify, scan, mark, offsets, edges, walk), against the sequential machine of pwm_host.hpp:
//   the composition table of the four maps (associativity, identity, agreement with applying one map after the other);
//   EVERY string of the four sample classes up to EXH_LEN samples, whole and cut in two at every point, under tiny settings
//   (short 1, long 2 or 3, tolerance 0 and 1, frame gap 2, reset gap 2 and 3, both gap modes);
//   drawn pulse trains over several tiles in random pushes, pushes of one sample included, with a flush at the end;
//   drawn transmissions of hundreds of frames of up to 70 bits against a table of 100 rows, cut at random and on every tile seam,
//   so pwm_step's order of find, append and turn away holds where the table is larger than one wave of the walk.
// Frames are compared exactly (bits, repeats, first_sample, order, and the push they are delivered in); so is the carried state.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pwm_host.hpp"

using namespace rr;

static int fails = 0;
static long delivered = 0, repeated = 0;     // frames the reference delivered in all comparisons; those with repeats > 1
static size_t max_carried = 0, max_open = 0; // the most candidates, and the longest open frame, that a push left to the next
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: %s — ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the device side of a handle: what it carries, and the kernels' work of one push
struct EmuOps {
    const PwmCfg& c;
    std::vector<unsigned char>& fbits;
    std::vector<PwmCand>& meta;
    std::vector<std::vector<unsigned char>>& rows;
    std::vector<PwmHostFrame>& out;
    void put_bit(unsigned idx, unsigned bit) { fbits[idx] = (unsigned char)bit; }
    void candidate(unsigned len, pwm_u64 first, pwm_u64 hash) {
        for (size_t i = 0; i < meta.size(); i++) {
            if (meta[i].len != len || meta[i].hash != hash) continue;
            if (std::equal(rows[i].begin(), rows[i].end(), fbits.begin())) { meta[i].repeats++; return; }
        }
        if (meta.size() < c.max_distinct) {
            meta.push_back(PwmCand{first, hash, len, 1});
            rows.emplace_back(fbits.begin(), fbits.begin() + len);
        }
    }
    void deliver() {
        for (size_t i = 0; i < meta.size(); i++) {
            if (meta[i].repeats < c.min_repeats) continue;
            PwmHostFrame f;
            f.bits = rows[i]; f.repeats = meta[i].repeats; f.first_sample = meta[i].first;
            out.push_back(f);
        }
        meta.clear();
        rows.clear();
    }
};
struct EmuDecoder {
    PwmCfg c;
    PwmState st{};
    std::vector<unsigned char> fbits;
    std::vector<PwmCand> meta;
    std::vector<std::vector<unsigned char>> rows;
    explicit EmuDecoder(const PwmCfg& cfg) : c(cfg), fbits(cfg.max_bits) {}
    void push(const float* p, size_t n, bool eof, std::vector<PwmHostFrame>& out) {
        const size_t ntiles = (n + PWM_T - 1) / PWM_T;
        // k_pwm_classify: one 16-bit word per thread, one map per tile
        std::vector<unsigned> cls(ntiles * PWM_B, 0), tmap(ntiles), tstate(ntiles), ebits(ntiles * PWM_B, 0), tilecnt(ntiles), offs(ntiles);
        for (size_t t = 0; t < ntiles; t++) {
            unsigned m = PWM_ID;
            // (the threads behind the push's last sample hold identities only: skipped, they change nothing)
            const int nth = (int)std::min<size_t>(PWM_B, (n - t * PWM_T + PWM_PER - 1) / PWM_PER);
            for (int th = 0; th < nth; th++) {
                unsigned c16 = 0;
                for (int i = 0; i < PWM_PER; i++) {
                    const size_t j = t * PWM_T + (size_t)th * PWM_PER + i;
                    c16 |= (j < n ? pwm_class(p[j], c.high_thr, c.low_thr) : PWM_ID) << (2 * i);
                }
                cls[t * PWM_B + th] = c16;
                m = pwm_compose(m, pwm_compose8(c16));
            }
            tmap[t] = m;
        }
        // k_pwm_scan
        unsigned state = st.high ? 1u : 0u;
        for (size_t t = 0; t < ntiles; t++) { tstate[t] = state; state = pwm_apply(tmap[t], state); }
        // k_pwm_mark, k_pwm_offs, k_pwm_edges
        unsigned total = 0;
        for (size_t t = 0; t < ntiles; t++) {
            unsigned m = PWM_ID, cnt = 0;
            const int nth = (int)std::min<size_t>(PWM_B, (n - t * PWM_T + PWM_PER - 1) / PWM_PER);
            for (int th = 0; th < nth; th++) {
                const unsigned c16 = cls[t * PWM_B + th], s0 = pwm_apply(m, tstate[t]);
                const unsigned e8 = pwm_edges8(pwm_states8(c16, s0), s0);
                ebits[t * PWM_B + th] = e8;
                cnt += (unsigned)__builtin_popcount(e8);
                m = pwm_compose(m, pwm_compose8(c16));
            }
            tilecnt[t] = cnt;
            offs[t] = total;
            total += cnt;
        }
        std::vector<unsigned> E(total + 1);
        for (size_t t = 0; t < ntiles; t++) {
            unsigned at = offs[t];
            for (int th = 0; th < PWM_B; th++)
                for (int i = 0; i < PWM_PER; i++)
                    if (ebits[t * PWM_B + th] >> i & 1) E[at++] = (unsigned)(t * PWM_T + (size_t)th * PWM_PER + i);
        }
        // k_pwm_walk
        const pwm_u64 ne = eof ? 0 : total;
        EmuOps ops{c, fbits, meta, rows, out};
        PwmWalk w;
        pwm_walk_load(w, st);
        const pwm_u64 nitems = pwm_items(st, ne);
        for (pwm_u64 j = 0; j < nitems; j++) pwm_step(c, w, pwm_item(c, st, E.data(), ne, n, j), ops);
        pwm_walk_tail(w, st, E.data(), ne);
        if (eof) ops.deliver();
        PwmState o;
        pwm_state_out(o, st, w, E.data(), ne, n, (unsigned)meta.size(), eof ? 1u : 0u);
        st = o;
    }
};

static const float CLASS_VALUE[4] = {0.0f, NAN, 0.375f, 1.0f};       // PWM_LOW, PWM_SWAP, PWM_ID, PWM_HIGH under 0.5 / 0.25

// the same samples through both, cut into the given pushes; flush at the end
static void compare(const PwmCfg& c, const std::vector<float>& x, const std::vector<size_t>& cuts, const char* what) {
    PwmMachine ref(c);
    EmuDecoder emu(c);
    size_t at = 0;
    for (size_t k = 0; k <= cuts.size(); k++) {
        const size_t end = k < cuts.size() ? cuts[k] : x.size();
        std::vector<PwmHostFrame> a, b;
        ref.push(x.data() + at, end - at, a);
        for (const auto& f : a) { delivered++; repeated += f.repeats > 1; }
        if (end > at) emu.push(x.data() + at, end - at, false, b);
        CHECK(a == b, "%s: push %zu of [%zu, %zu): %zu frames against %zu", what, k, at, end, b.size(), a.size());
        CHECK(emu.st.pos == ref.sample_index && (emu.st.high != 0) == ref.high && emu.st.run == (ref.high ? ref.high_run : ref.low_run),
              "%s: carried slicer state behind %zu", what, end);
        if (!ref.frame_invalid && !ref.bits.empty())
            CHECK(emu.st.fcount == ref.bits.size() && !emu.st.finvalid && emu.st.has_start && emu.st.fstart == ref.frame_start,
                  "%s: carried frame behind %zu", what, end);
        CHECK(emu.meta.size() == ref.candidates.size(), "%s: carried candidates behind %zu", what, end);
        max_carried = std::max(max_carried, ref.candidates.size());
        max_open = std::max(max_open, ref.bits.size());
        at = end;
    }
    std::vector<PwmHostFrame> a, b;
    ref.finish_transmission(a);
    emu.push(nullptr, 0, true, b);
    CHECK(a == b, "%s: flush: %zu frames against %zu", what, b.size(), a.size());
}

static PwmCfg tiny(unsigned long_w, unsigned tol, unsigned rgap, int delimiter, unsigned max_bits, unsigned max_distinct, unsigned frame_bits) {
    return pwm_cfg(0.5f, 0.25f, 1, long_w, tol, 2, rgap, frame_bits, max_bits, max_distinct, 1, delimiter ? RR_PWM_GAP_DELIMITER : 0);
}

int main(int argc, char** argv) {
    const int EXH_LEN = argc > 1 ? std::atoi(argv[1]) : 7;
    // ---- the four maps
    for (unsigned a = 0; a < 4; a++) {
        CHECK(pwm_compose(a, PWM_ID) == a && pwm_compose(PWM_ID, a) == a, "identity");
        for (unsigned b = 0; b < 4; b++) {
            for (unsigned s = 0; s < 2; s++) CHECK(pwm_apply(pwm_compose(a, b), s) == pwm_apply(b, pwm_apply(a, s)), "compose is b after a");
            for (unsigned d = 0; d < 4; d++) CHECK(pwm_compose(pwm_compose(a, b), d) == pwm_compose(a, pwm_compose(b, d)), "associativity");
        }
    }
    CHECK(pwm_class(1.0f, 0.5f, 0.25f) == PWM_HIGH && pwm_class(0.0f, 0.5f, 0.25f) == PWM_LOW && pwm_class(0.5f, 0.5f, 0.25f) == PWM_ID &&
          pwm_class(0.25f, 0.5f, 0.25f) == PWM_ID && pwm_class(NAN, 0.5f, 0.25f) == PWM_SWAP && pwm_class(INFINITY, 0.5f, 0.25f) == PWM_HIGH &&
          pwm_class(-INFINITY, 0.5f, 0.25f) == PWM_LOW, "classes on and off the thresholds");
    // ---- every string of classes
    long runs = 0;
    for (unsigned long_w = 2; long_w <= 3; long_w++)
        for (unsigned tol = 0; tol <= 1; tol++)
            for (unsigned rgap = 2; rgap <= 3; rgap++)
                for (int delim = 0; delim <= 1; delim++) {
                    const PwmCfg c = tiny(long_w, tol, rgap, delim, 2, 2, 0);
                    for (int len = 0; len <= EXH_LEN; len++) {
                        std::vector<float> x(len);
                        for (unsigned long code = 0; code < 1ul << (2 * len); code++) {
                            for (int i = 0; i < len; i++) x[i] = CLASS_VALUE[code >> (2 * i) & 3];
                            // strings of the full length whole only beyond EXH_LEN - 1; shorter ones at every cut
                            if (len == EXH_LEN) { compare(c, x, {}, "exhaustive"); runs++; continue; }
                            for (int cut = 0; cut <= len; cut++) { compare(c, x, {(size_t)cut}, "exhaustive, cut"); runs++; }
                        }
                    }
                }
    // ---- drawn trains over several tiles
    std::mt19937_64 rng(12345);
    for (int round = 0; round < 60; round++) {
        const bool delim = round & 1;
        const unsigned fb = round % 5 == 0 ? 4 : 0;
        const PwmCfg c = pwm_cfg(0.5f, 0.25f, 3, 7, round % 3, 12, round % 4 == 0 ? 12 : 30, fb, 6, 3, 1 + round % 2, (delim ? RR_PWM_GAP_DELIMITER : 0) | (round & 2 ? RR_PWM_SHORT_IS_ZERO : 0));
        std::vector<float> x;
        const size_t target = 2 * PWM_T + 700 + (size_t)(rng() % 3000);
        while (x.size() < target) {
            const unsigned kind = (unsigned)(rng() % 16);
            const size_t w = kind < 8 ? (rng() % 2 ? 3 : 7) + (size_t)(rng() % 3) - 1 : kind < 10 ? (size_t)(rng() % 12) : (rng() % 2 ? 3 : 7);
            const size_t g = kind < 11 ? 2 + (size_t)(rng() % 5) : kind < 14 ? 11 + (size_t)(rng() % 3) : 29 + (size_t)(rng() % 3);
            for (size_t i = 0; i < w; i++) x.push_back(rng() % 9 == 0 ? 0.3f : 1.0f);
            for (size_t i = 0; i < g; i++) x.push_back(rng() % 9 == 0 ? 0.4f : rng() % 97 == 0 ? NAN : 0.0f);
        }
        compare(c, x, {}, "drawn, whole");
        std::vector<size_t> cuts;
        for (size_t at = 0; at < x.size();) { at += 1 + (size_t)(rng() % (round % 2 ? 40 : 3000)); if (at < x.size()) cuts.push_back(at); }
        compare(c, x, cuts, "drawn, cut");
        for (size_t seam : {(size_t)PWM_T - 1, (size_t)PWM_T, (size_t)PWM_T + 1}) compare(c, x, {seam}, "drawn, cut at a tile seam");
        runs += 5;
    }
    // ---- drawn transmissions against a table of 100 rows: a pool of 140 words, most of 1 .. 12 bits, a quarter of 1 .. 71 (one more
    // than max_frame_bits), 260 frames a transmission, so the table fills and turns words away; some 7,000 pulses a round
    for (int round = 0; round < 4; round++) {
        const bool delim = round & 1;
        const PwmCfg c = pwm_cfg(0.5f, 0.25f, 1, 3, (round >> 1) & 1, 5, 12, 0, 70, 100, 1 + round % 2,
                                 (delim ? RR_PWM_GAP_DELIMITER : 0) | (round & 2 ? RR_PWM_SHORT_IS_ZERO : 0));
        std::vector<std::vector<unsigned char>> pool(140);
        for (auto& wd : pool) {
            wd.resize(rng() % 4 == 0 ? 1 + (size_t)(rng() % 71) : 1 + (size_t)(rng() % 12));
            for (auto& b : wd) b = (unsigned char)(rng() % 2);
        }
        std::vector<float> x;
        auto run = [&](bool high, size_t count) {          // (inside the band behind the run's first sample only: the widths stand)
            for (size_t i = 0; i < count; i++) x.push_back(high ? (i && rng() % 9 == 0 ? 0.3f : 1.0f) : (i && rng() % 9 == 0 ? 0.4f : 0.0f));
        };
        for (int tx = 0; tx < 2; tx++) {
            for (int f = 0; f < 260; f++) {
                for (unsigned char b : pool[rng() % pool.size()]) {
                    run(true, rng() % 50 == 0 ? 2 : b ? 1 : 3);      // a width of 2: the tie under tolerance 1, invalid under 0
                    run(false, 1 + (size_t)(rng() % 4));
                }
                if (delim) run(true, 1);
                run(false, f == 259 ? 12 + (size_t)(rng() % 3) : 5 + (size_t)(rng() % 7));
            }
        }
        compare(c, x, {}, "table of 100, whole");
        std::vector<size_t> cuts, seams, beside;
        for (size_t at = 0; at < x.size();) { at += 1 + (size_t)(rng() % (round % 2 ? 40 : 3000)); if (at < x.size()) cuts.push_back(at); }
        compare(c, x, cuts, "table of 100, cut");
        for (size_t at = PWM_T; at + 1 < x.size(); at += PWM_T) { seams.push_back(at); beside.push_back(at - 1); beside.push_back(at + 1); }
        compare(c, x, seams, "table of 100, cut on every tile seam");
        compare(c, x, beside, "table of 100, cut beside every tile seam");
        runs += 4;
    }
    CHECK(max_carried == 100 && max_open > 64, "a full table of 100 and an open frame past 64 bits are carried: %zu, %zu", max_carried, max_open);
    CHECK(delivered > 10000 && repeated > 100, "the comparisons deliver frames: %ld, %ld repeated", delivered, repeated);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("%ld comparisons, %ld frames delivered, %ld of them repeated\npwm core ok\n", runs, delivered, repeated);
    return 0;
}
