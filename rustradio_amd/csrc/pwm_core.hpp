// pwm_core.hpp — the arithmetic the kernels of kernels_pwm.hip share with the host: plain functions, no HIP types, so
// tests/cpp/emu_pwm.cpp compiles them with g++ and holds them to the reference's sequential machine.
// PwmDecoder (src/pwm_decoder.rs:385-513) in closed form:
//   pwm_class / pwm_compose    a sample as one of the four maps on {low, high}, and their composition
//   pwm_pulse                  short, long or invalid from a width (:434-446)
//   pwm_item                   one fall of the push (or the low run the stream so far left open): its pulse, whether it is data,
//                              and whether the frame-gap and the reset event fire behind it inside this push
//   pwm_step                   what one item does to the open frame, the candidates and the deliveries (:447-513)
// Positions are absolute sample positions as 64-bit counts; an edge list holds positions relative to the push.
#pragma once

#if defined(__HIPCC__)
#define RR_PWM_HD __host__ __device__ inline
#else
#define RR_PWM_HD inline
#endif

namespace rr {

typedef unsigned long long pwm_u64;

constexpr int PWM_B = 256, PWM_PER = 8;       // threads of a tile's workgroup; consecutive samples of one thread
constexpr int PWM_T = PWM_B * PWM_PER;        // samples of a tile
constexpr int PWM_SB = 1024;                  // tiles of one chunk of the two one-workgroup scans
static_assert(PWM_PER == 8, "a thread's classes are one 16-bit word, its edges one byte");

// ---- the four maps --------------------------------------------------------------------------------------------------------------------
// bit 0: the state behind the sample when it was low in front of it, bit 1: when it was high.
constexpr unsigned PWM_LOW = 0, PWM_SWAP = 1, PWM_ID = 2, PWM_HIGH = 3;
// :386-396 — in low, p <= high_threshold stays low; in high, p >= low_threshold stays high.  A NaN fails both: it swaps.
RR_PWM_HD unsigned pwm_class(float p, float high_thr, float low_thr) {
    const unsigned from_low = p <= high_thr ? 0u : 1u, from_high = p >= low_thr ? 1u : 0u;
    return from_low | from_high << 1;
}
RR_PWM_HD unsigned pwm_apply(unsigned m, unsigned state) { return (m >> state) & 1u; }
// first a, then b
RR_PWM_HD unsigned pwm_compose(unsigned a, unsigned b) { return pwm_apply(b, a & 1u) | pwm_apply(b, (a >> 1) & 1u) << 1; }
// the map of a thread's PWM_PER samples, oldest in the low bits
RR_PWM_HD unsigned pwm_compose8(unsigned c16) {
    unsigned m = PWM_ID;
    for (int i = 0; i < PWM_PER; ++i) m = pwm_compose(m, (c16 >> (2 * i)) & 3u);
    return m;
}
// the states behind each of the thread's samples (bit i) from the state in front of the first
RR_PWM_HD unsigned pwm_states8(unsigned c16, unsigned state) {
    unsigned out = 0;
    for (int i = 0; i < PWM_PER; ++i) {
        state = pwm_apply((c16 >> (2 * i)) & 3u, state);
        out |= state << i;
    }
    return out;
}
// bit i: sample i's state differs from the one in front of it
RR_PWM_HD unsigned pwm_edges8(unsigned states, unsigned state_in_front) { return (states ^ (states << 1 | state_in_front)) & 0xffu; }

// ---- settings and what a handle carries --------------------------------------------------------------------------------------------
struct PwmCfg {
    float high_thr, low_thr;
    pwm_u64 short_w, long_w, tol, fgap, rgap;
    unsigned frame_bits;                      // 0: None
    unsigned max_bits, max_distinct, min_repeats;
    int short_is_one, delimiter;
};
struct PwmState {
    pwm_u64 pos;                              // samples of the stream so far
    pwm_u64 run;                              // length of the high or low run that is open
    pwm_u64 pending_w;                        // the pulse behind which neither a rise nor the frame gap has come yet
    pwm_u64 fstart, fhash;                    // the open frame: its first rise, the hash of its bits
    unsigned high, has_pending, fcount, finvalid, has_start, ncand, eof, pad;
};
// one candidate's numbers; its bits stand in the candidate table, `pitch` bytes per row
struct PwmCand {
    pwm_u64 first, hash;
    unsigned len, repeats;
};
struct PwmRec {                               // rr_pwm_frame
    pwm_u64 first_sample, start;
    unsigned len, repeats;
};
RR_PWM_HD pwm_u64 pwm_pitch(unsigned max_bits) { return ((pwm_u64)max_bits + 7) & ~7ull; }
RR_PWM_HD pwm_u64 pwm_hash_step(pwm_u64 h, unsigned bit) { return (h ^ (bit + 1u)) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull; }

// 0 short, 1 long, 2 invalid (:434-446)
RR_PWM_HD int pwm_pulse(const PwmCfg& c, pwm_u64 w) {
    const pwm_u64 ds = w > c.short_w ? w - c.short_w : c.short_w - w, dl = w > c.long_w ? w - c.long_w : c.long_w - w;
    const bool sv = ds <= c.tol, lv = dl <= c.tol;
    if (sv && lv) return ds <= dl ? 0 : 1;
    return sv ? 0 : lv ? 1 : 2;
}

// ---- one item ---------------------------------------------------------------------------------------------------------------------------
constexpr unsigned PWM_IT_DATA = 1, PWM_IT_BIT = 2, PWM_IT_BAD = 4, PWM_IT_END = 8, PWM_IT_RESET = 16, PWM_IT_OPEN = 32, PWM_IT_RISE = 64,
                   PWM_IT_PULSE = 128;
struct PwmItem {
    unsigned flags;
    pwm_u64 rise, width;
};
// items of a push whose edge list has ne entries: every fall, and in front of them the low run the stream so far left open
RR_PWM_HD pwm_u64 pwm_items(const PwmState& st, pwm_u64 ne) { return st.high ? (ne + 1) / 2 : 1 + ne / 2; }
// The gap event of length G behind a fall: low_run EQUALS G at sample fall + G - 1, on a sample that stays low (:397-409), so
// never on the fall itself (G >= 2).  It fires in this push when that sample lies in [pos, pos + n) and in front of the next rise.
// since = pos - fall for the carried run (0 for a fall of this push), left = pos + n - fall, gap = the low run's length if a rise ends it.
RR_PWM_HD bool pwm_fires(pwm_u64 G, pwm_u64 since, pwm_u64 left, bool next, pwm_u64 gap) {
    return G >= 2 && G - 1 >= since && G - 1 < left && (!next || gap > G - 1);
}
// item j of the push of n samples at st.pos; E: the push's edges in stream order, relative, alternating from !st.high
RR_PWM_HD PwmItem pwm_item(const PwmCfg& c, const PwmState& st, const unsigned* E, pwm_u64 ne, pwm_u64 n, pwm_u64 j) {
    const long long k = 2 * (long long)j - (st.high ? 0 : 1);        // the fall's place in E; -1: the carried low run
    PwmItem it;
    it.flags = 0; it.rise = 0; it.width = 0;
    pwm_u64 since = 0, left, fall_rel = 0;
    bool pulse = true;
    if (k < 0) {
        since = st.run;
        left = st.run + n;
        pulse = st.has_pending != 0;
        it.width = st.pending_w;
    } else {
        fall_rel = E[k];
        left = n - fall_rel;
        if (k >= 1) {
            it.rise = st.pos + E[k - 1];
            it.width = (pwm_u64)E[k] - E[k - 1];
            it.flags |= PWM_IT_RISE;
        } else {
            it.width = st.run + fall_rel;                            // the high run the stream so far left open
        }
    }
    const bool next = (pwm_u64)(k + 1) < ne;
    const pwm_u64 gap = next ? (k < 0 ? st.run + E[k + 1] : (pwm_u64)E[k + 1] - fall_rel) : 0;
    const bool fend = pwm_fires(c.fgap, since, left, next, gap), freset = pwm_fires(c.rgap, since, left, next, gap);
    if (pulse) it.flags |= PWM_IT_PULSE;
    if (pulse && ((next && gap < c.fgap) || (fend && !c.delimiter))) {   // :412-413 at the rise, :399-402 at the gap
        const int cls = pwm_pulse(c, it.width);
        it.flags |= PWM_IT_DATA;
        if (cls == 2) it.flags |= PWM_IT_BAD;
        else if ((cls == 0) == (c.short_is_one != 0)) it.flags |= PWM_IT_BIT;
    }
    if (fend) it.flags |= PWM_IT_END;
    if (freset) it.flags |= PWM_IT_RESET;
    if (!next && !fend) it.flags |= PWM_IT_OPEN;
    return it;
}

// ---- what an item does --------------------------------------------------------------------------------------------------------------
// The open frame between items.  Ops: put_bit(index, bit), candidate(len, first_sample, hash) (finish_frame's find-or-push,
// :485-497) and deliver() (finish_transmission, :502-513).
struct PwmWalk {
    pwm_u64 fstart, fhash, pending_w;
    unsigned fcount, finvalid, has_start, has_pending;
};
RR_PWM_HD void pwm_walk_load(PwmWalk& w, const PwmState& st) {
    w.fstart = st.fstart; w.fhash = st.fhash; w.pending_w = 0;
    w.fcount = st.fcount; w.finvalid = st.finvalid; w.has_start = st.has_start; w.has_pending = 0;
}
RR_PWM_HD void pwm_walk_clear(PwmWalk& w) { w.fcount = 0; w.finvalid = 0; w.has_start = 0; w.fhash = 0; }
template <class Ops> RR_PWM_HD void pwm_step(const PwmCfg& c, PwmWalk& w, const PwmItem& it, Ops& ops) {
    // :420-422 — the first rise of a frame is its start (a frame that is invalid by then is never delivered)
    if ((it.flags & PWM_IT_RISE) && !w.has_start) { w.fstart = it.rise; w.has_start = 1; }
    if ((it.flags & PWM_IT_OPEN) && (it.flags & PWM_IT_PULSE)) { w.has_pending = 1; w.pending_w = it.width; }
    if ((it.flags & PWM_IT_DATA) && !w.finvalid) {
        if ((it.flags & PWM_IT_BAD) || w.fcount == c.max_bits) {      // :442-450 — an invalidated frame stays rejected up to its gap
            w.finvalid = 1;
        } else {
            const unsigned bit = it.flags & PWM_IT_BIT ? 1u : 0u;
            ops.put_bit(w.fcount, bit);
            w.fhash = pwm_hash_step(w.fhash, bit);
            w.fcount++;
        }
    }
    if (it.flags & PWM_IT_END) {                                      // :471-499
        if (!w.finvalid && w.fcount >= 1 && (c.frame_bits == 0 || w.fcount == c.frame_bits)) ops.candidate(w.fcount, w.fstart, w.fhash);
        pwm_walk_clear(w);
    }
    if (it.flags & PWM_IT_RESET) {
        ops.deliver();
        pwm_walk_clear(w);
    }
}
// behind the last item: a rise of this push that no fall has followed yet starts a frame as well
RR_PWM_HD void pwm_walk_tail(PwmWalk& w, const PwmState& st, const unsigned* E, pwm_u64 ne) {
    const bool high_end = ((st.high ? 1u : 0u) ^ (unsigned)(ne & 1)) != 0;
    if (high_end && ne && !w.has_start) { w.fstart = st.pos + E[ne - 1]; w.has_start = 1; }
}
RR_PWM_HD void pwm_state_out(PwmState& o, const PwmState& st, const PwmWalk& w, const unsigned* E, pwm_u64 ne, pwm_u64 n, unsigned ncand,
                             unsigned eof) {
    o.pos = st.pos + n;
    o.high = (st.high ? 1u : 0u) ^ (unsigned)(ne & 1);
    o.run = ne ? n - E[ne - 1] : st.run + n;
    o.has_pending = o.high ? 0u : w.has_pending;
    o.pending_w = o.has_pending ? w.pending_w : 0;
    o.fstart = w.fstart; o.fhash = w.fhash;
    o.fcount = w.fcount; o.finvalid = w.finvalid; o.has_start = w.has_start;
    o.ncand = ncand; o.eof = eof; o.pad = 0;
}

}  // namespace rr
