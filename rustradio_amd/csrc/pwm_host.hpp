// pwm_host.hpp — the host-only logic behind rr_pwm_decoder_create / _push / _push_dev / _flush, rr_pwm_frames and
// rr_pwm_frame_bits: the refusals (validate(), src/pwm_decoder.rs:101-162, in its words, and the limits of a handle), the
// workspace plan of a push, the validation of everything the device wrote, the clamped copy-outs — and PwmMachine, the
// reference's sequential machine (:385-513) sample by sample, which tests/cpp/emu_pwm.cpp holds pwm_core.hpp to and
// tools/pwm_probe.py times as the path the device block replaces.  No HIP in here.  Every host buffer is sized from the push
// length and the settings, never from a number the device wrote; what the device wrote is checked against those bounds BEFORE it
// is used as a size or an index.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rustradio_amd.h"
#include "pwm_core.hpp"

namespace rr {

constexpr size_t PWM_MAX_PUSH = (size_t)1 << 30;          // samples of one push
constexpr size_t PWM_MAX_FRAME_BITS = 16384, PWM_MAX_DISTINCT = 1024, PWM_MAX_TABLE = (size_t)1 << 22;
constexpr unsigned long long PWM_MAX_WIDTH = 1ull << 62;
constexpr int PWM_ALL_FLAGS = RR_PWM_SHORT_IS_ZERO | RR_PWM_GAP_DELIMITER;
static_assert(sizeof(rr_pwm_frame) == 24 && sizeof(PwmRec) == 24, "rr_pwm_frame is 24 bytes");
static_assert(offsetof(PwmRec, first_sample) == offsetof(rr_pwm_frame, first_sample) && offsetof(PwmRec, start) == offsetof(rr_pwm_frame, start) &&
              offsetof(PwmRec, len) == offsetof(rr_pwm_frame, len) && offsetof(PwmRec, repeats) == offsetof(rr_pwm_frame, repeats),
              "PwmRec is rr_pwm_frame");

// What rr_pwm_decoder_create refuses, said before any device is touched; nullptr: fine.  validate() first, in its order.
inline const char* pwm_check_create(float high, float low, size_t short_w, size_t long_w, size_t tol, size_t fgap, size_t rgap,
                                    size_t frame_bits, size_t max_bits, size_t max_distinct, size_t min_repeats, int flags, size_t es) {
    if (!std::isfinite(high) || high <= 0.0f) return "PwmDecoder high threshold must be finite and greater than zero";
    if (!std::isfinite(low) || low <= 0.0f || low > high)
        return "PwmDecoder low threshold must be finite, greater than zero, and no greater than the high threshold";
    if (short_w == 0) return "PwmDecoder short pulse width must be greater than zero";
    if (long_w <= short_w) return "PwmDecoder long pulse width must be greater than the short pulse width";
    if (fgap == 0) return "PwmDecoder frame gap must be greater than zero";
    if (rgap < fgap) return "PwmDecoder reset gap must be at least as long as the frame gap";
    // (frame_bits == Some(0) cannot be said through this call: 0 is None)
    if (max_bits == 0) return "PwmDecoder maximum frame length must be greater than zero";
    if (frame_bits > max_bits) return "PwmDecoder fixed frame length exceeds the maximum frame length";
    if (max_distinct == 0) return "PwmDecoder maximum distinct frames must be greater than zero";
    if (min_repeats == 0) return "PwmDecoder minimum repeats must be greater than zero";
    if (flags & ~PWM_ALL_FLAGS) return "unknown pwm decoder flags";
    if (es != 4 && es != 8) return "pwm decoder: Float (4) or Complex (8) input only";
    if (max_bits > PWM_MAX_FRAME_BITS) return "pwm decoder: max_frame_bits beyond 16384";
    if (max_distinct > PWM_MAX_DISTINCT) return "pwm decoder: max_distinct_frames beyond 1024";
    if (max_bits * max_distinct > PWM_MAX_TABLE) return "pwm decoder: max_frame_bits x max_distinct_frames beyond 4194304";
    if (long_w > PWM_MAX_WIDTH || tol > PWM_MAX_WIDTH || rgap > PWM_MAX_WIDTH) return "pwm decoder: width or gap beyond 2^62";
    if (min_repeats > 0xffffffffull) return "pwm decoder: min_repeats beyond 2^32 - 1";
    return nullptr;
}
inline PwmCfg pwm_cfg(float high, float low, size_t short_w, size_t long_w, size_t tol, size_t fgap, size_t rgap, size_t frame_bits,
                      size_t max_bits, size_t max_distinct, size_t min_repeats, int flags) {
    PwmCfg c{};
    c.high_thr = high; c.low_thr = low;
    c.short_w = short_w; c.long_w = long_w; c.tol = tol; c.fgap = fgap; c.rgap = rgap;
    c.frame_bits = (unsigned)frame_bits; c.max_bits = (unsigned)max_bits; c.max_distinct = (unsigned)max_distinct;
    c.min_repeats = (unsigned)min_repeats;
    c.short_is_one = flags & RR_PWM_SHORT_IS_ZERO ? 0 : 1;
    c.delimiter = flags & RR_PWM_GAP_DELIMITER ? 1 : 0;
    return c;
}
// What a push refuses (nothing may be launched then); nullptr: fine.
inline const char* pwm_check_push(const void* samples, size_t n, bool flushed) {
    if (flushed) return "pwm decoder: push after flush";
    if (n > PWM_MAX_PUSH) return "pwm decoder: more than 2^30 samples in one push";
    if (n && !samples) return "pwm decoder: null samples";
    return nullptr;
}

// The workspace and the bounds of a push of n samples (n == 0: a flush), in the units the kernels index by (PwmArgs).
struct PwmPlan {
    size_t ntiles = 0;    // tiles of PWM_T samples: tmap / tstate / tilecnt / offs
    size_t nthreads = 0;  // cls / ebits: one per thread of every tile
    size_t ecap = 0;      // edges: one per sample at most
    size_t frames = 0;    // records: the carried candidates and one frame per pulse of the push and the pending one
    size_t arena = 0;     // their bits: the carried table, the carried open frame and one bit per pulse
};
inline PwmPlan pwm_plan(size_t n, size_t max_bits, size_t max_distinct) {
    PwmPlan p;
    p.ntiles = (n + PWM_T - 1) / PWM_T;
    p.nthreads = p.ntiles * PWM_B;
    p.ecap = n;
    p.frames = max_distinct + (n ? n / 2 + 2 : 0);
    p.arena = max_distinct * max_bits + (n ? max_bits + n / 2 + 2 : 0);
    return p;
}

// The two counts the device left, before they size anything.
inline const char* pwm_check_counts(unsigned long long frames, unsigned long long bits, const PwmPlan& p) {
    if (frames > p.frames) return "pwm decoder: frame count beyond the bound";
    if (bits > p.arena) return "pwm decoder: bit count beyond the bound";
    return nullptr;
}
// The records of a push that ended at stream position `end`, in delivery order: nullptr, or why the device's numbers cannot be
// trusted (then rec is empty).  Frames stand one behind the other in the arena.
inline const char* pwm_validate(std::vector<rr_pwm_frame>& rec, unsigned long long bits, const PwmPlan& p, size_t max_bits, size_t min_repeats,
                                unsigned long long end) {
    const char* bad = nullptr;
    if (rec.size() > p.frames || bits > p.arena) bad = "pwm decoder: frame count beyond the bound";
    unsigned long long at = 0;
    for (size_t i = 0; i < rec.size() && !bad; i++) {
        const rr_pwm_frame& r = rec[i];
        if (r.len == 0 || r.len > max_bits) bad = "pwm decoder: frame length outside 1 .. max_frame_bits";
        else if (r.start != at || r.len > bits - at) bad = "pwm decoder: frame outside the arena";
        else if (r.repeats < min_repeats) bad = "pwm decoder: frame below min_repeats";
        else if (r.first_sample >= end) bad = "pwm decoder: first sample beyond the push";
        at += r.len;
    }
    if (!bad && at != bits) bad = "pwm decoder: bit count and frame lengths disagree";
    if (bad) rec.clear();
    return bad;
}
inline const char* pwm_validate_bits(const std::vector<unsigned char>& bits) {
    for (unsigned char b : bits)
        if (b > 1) return "pwm decoder: a bit that is neither 0 nor 1";
    return nullptr;
}

// The contract of rr_hdlc_frames: *total = all, the first min(all, cap) copied; out may be NULL with cap == 0.
inline void pwm_copy_frames(const std::vector<rr_pwm_frame>& r, rr_pwm_frame* out, size_t cap, size_t* total) {
    *total = r.size();
    const size_t k = std::min(cap, r.size());
    if (k && out) std::memcpy(out, r.data(), k * sizeof(rr_pwm_frame));
}
inline void pwm_copy_bits(const std::vector<unsigned char>& a, unsigned char* out, size_t cap, size_t* total) {
    *total = a.size();
    const size_t k = std::min(cap, a.size());
    if (k && out) std::memcpy(out, a.data(), k);
}

// ---- the reference's machine, sample by sample (:385-513) -------------------------------------------------------------------------------
struct PwmHostFrame {
    std::vector<unsigned char> bits;
    unsigned long long repeats = 0, first_sample = 0;
    bool operator==(const PwmHostFrame& o) const { return bits == o.bits && repeats == o.repeats && first_sample == o.first_sample; }
};
struct PwmMachine {
    PwmCfg c;
    unsigned long long sample_index = 0, high_run = 0, low_run = 0, pending = 0, frame_start = 0;
    bool high = false, has_pending = false, has_start = false, frame_invalid = false;
    std::vector<unsigned char> bits;
    std::vector<PwmHostFrame> candidates;
    explicit PwmMachine(const PwmCfg& cfg) : c(cfg) {}
    void finish_pending_pulse() {
        if (!has_pending) return;
        has_pending = false;
        const int cls = pwm_pulse(c, pending);
        if (cls == 2 || bits.size() == c.max_bits) { invalidate_frame(); return; }
        bits.push_back((unsigned char)((cls == 0) == (c.short_is_one != 0) ? 1 : 0));
    }
    void invalidate_frame() { bits.clear(); has_start = false; frame_invalid = true; }
    void clear_frame() { bits.clear(); has_start = false; frame_invalid = false; has_pending = false; }
    void finish_frame() {
        if (frame_invalid || bits.empty() || (c.frame_bits && c.frame_bits != bits.size())) { clear_frame(); return; }
        const unsigned long long first = has_start ? frame_start : sample_index;
        bool found = false;
        for (auto& k : candidates)
            if (k.bits == bits) { k.repeats++; found = true; break; }
        if (!found && candidates.size() < c.max_distinct) {
            PwmHostFrame f;
            f.bits = bits; f.repeats = 1; f.first_sample = first;
            candidates.push_back(f);
        }
        clear_frame();
    }
    void finish_transmission(std::vector<PwmHostFrame>& out) {
        clear_frame();
        for (auto& k : candidates)
            if (k.repeats >= c.min_repeats) out.push_back(k);
        candidates.clear();
    }
    void process(float p, std::vector<PwmHostFrame>& out) {
        if (high) {
            if (p >= c.low_thr) high_run++;
            else { high = false; has_pending = true; pending = high_run; high_run = 0; low_run = 1; }
        } else if (p <= c.high_thr) {
            low_run++;
            if (low_run == c.fgap) {
                if (c.delimiter) has_pending = false; else finish_pending_pulse();
                finish_frame();
            }
            if (low_run == c.rgap) finish_transmission(out);
        } else {
            if (low_run < c.fgap) finish_pending_pulse(); else has_pending = false;
            high = true; high_run = 1; low_run = 0;
            if (bits.empty() && !frame_invalid) { frame_start = sample_index; has_start = true; }
        }
        sample_index++;
    }
    // rr_pwm_decoder_push over n samples -> the frames delivered inside them, appended
    size_t push(const float* p, size_t n, std::vector<PwmHostFrame>& out) {
        const size_t k0 = out.size();
        for (size_t i = 0; i < n; i++) process(p[i], out);
        return out.size() - k0;
    }
};

}  // namespace rr
