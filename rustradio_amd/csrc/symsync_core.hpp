// symsync_core.hpp — the arithmetic k_sync_clock of kernels_sync.hip shares with the host: plain functions, no HIP types, so
// tests/cpp/emu_symsync.cpp compiles them with g++ -ffp-contract=off and holds them to the reference's sequential machine
// (DESIGN.md 4.16).  SymbolSync::work (src/symbol_sync.rs:115-217) with TedZeroCrossing and IirFilter::filter_clamped
// (src/iir_filter.rs:104-125), one sample per sync_step:
//   sync_derive   what the reference recomputes at every sign change from sps and max_deviation
//   sync_init     SymbolSync::new (:71-98), fill(sps) included
//   sync_step     one iteration of the `for sample in input.iter()` loop (:140-210), the sample reduced to `sample > 0.0`
//   sync_sign_word    the packing k_sync_signs does with a wave ballot
// Every f32 operation is one separately rounded operation in the reference's order: the device's kernels are built with
// -ffp-contract=fast, so there SYNC_MUL / SYNC_ADD / SYNC_SUB are common.hpp's mul_rn / add_rn / sub_rn; on the host they are the
// plain operators under -ffp-contract=off.
#pragma once
#if defined(__HIPCC__)
#define RR_SYNC_HD __host__ __device__ inline
#else
#define RR_SYNC_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SYNC_MUL(a, b) ::rr::mul_rn((a), (b))
#define SYNC_ADD(a, b) ::rr::add_rn((a), (b))
#define SYNC_SUB(a, b) ::rr::sub_rn((a), (b))
#else
#define SYNC_MUL(a, b) ((a) * (b))
#define SYNC_ADD(a, b) ((a) + (b))
#define SYNC_SUB(a, b) ((a) - (b))
#endif

namespace rr {

constexpr int SYNC_MAX_TAPS = 8;              // (a deviation: the reference has no cap; the examples use 2)

struct SyncParams {
    float sps, max_dev;
    float taps[SYNC_MAX_TAPS];
    int ntaps;
    float mx, t_lo, t_hi, c_lo, c_hi;         // sync_derive
};
// One stream's SymbolSync between two samples.
struct SyncState {
    float clock, stream_pos, last_sym_boundary_pos, next_sym_middle;
    int last_sign;
    float hist[SYNC_MAX_TAPS - 1];            // the filter's VecDeque, NEWEST first: ntaps - 1 entries, zeros behind them
};

RR_SYNC_HD float sync_abs(float x) { return x < 0.0f ? -x : x; }         // (-0.0 stays -0.0: only ever compared)

// :163-164, :174, :183-184 — host only (sps, max_dev and taps set by the caller)
inline void sync_derive(SyncParams& p) {
    const float mi = p.sps - p.max_dev;
    p.mx = p.sps + p.max_dev;
    p.t_lo = mi * 0.8f;
    p.t_hi = p.mx * 1.2f;
    p.c_lo = mi - p.sps;
    p.c_hi = p.mx - p.sps;
}
// :78-98 — host only.  fill(sps) puts ntaps - 1 copies of SPS into a history that otherwise holds deviations (iir_filter.rs:96-101)
inline void sync_init(SyncState& s, const SyncParams& p) {
    s.clock = p.sps;
    s.stream_pos = 0.0f;
    s.last_sym_boundary_pos = 0.0f;
    s.next_sym_middle = p.sps * 0.5f;
    s.last_sign = 0;
    for (int i = 0; i < SYNC_MAX_TAPS - 1; ++i) s.hist[i] = i < p.ntaps - 1 ? p.sps : 0.0f;
}

// iir_filter.rs:113-124
RR_SYNC_HD float sync_filter_clamped(SyncState& s, const SyncParams& p, float x) {
    const int nh = p.ntaps - 1;
    float r = SYNC_MUL(p.taps[0], x);
    // (constant trip counts and indices: the state stays in registers on the device)
#pragma unroll
    for (int i = 0; i < SYNC_MAX_TAPS - 1; ++i)
        if (i < nh) r = SYNC_ADD(r, SYNC_MUL(s.hist[i], p.taps[i + 1]));
    r = r < p.c_lo ? p.c_lo : (r > p.c_hi ? p.c_hi : r);
#pragma unroll
    for (int i = SYNC_MAX_TAPS - 2; i > 0; --i)         // push_back, pop_front
        if (i < nh) s.hist[i] = s.hist[i - 1];
    if (nh > 0) s.hist[0] = r;
    return r;
}

// One sample.  true: the sample is a symbol, and *clock_out the clock value that goes with it (:142-149).
RR_SYNC_HD bool sync_step(SyncState& s, const SyncParams& p, bool sign, float* clock_out) {
    bool emit = false;
    if (s.stream_pos >= s.next_sym_middle) {
        emit = true;
        *clock_out = s.clock;
        s.next_sym_middle = SYNC_ADD(s.next_sym_middle, s.clock);
    }
    if ((int)sign != s.last_sign) {
        if (s.stream_pos > 0.0f && s.last_sym_boundary_pos > 0.0f) {
            float t = SYNC_SUB(s.stream_pos, s.last_sym_boundary_pos);
            while (t > p.mx) {                                                                       // :167-173
                const float t2 = SYNC_SUB(t, s.clock);
                if (sync_abs(SYNC_SUB(t, s.clock)) < sync_abs(SYNC_SUB(t2, s.clock))) break;
                t = t2;
            }
            if (t > p.t_lo && t < p.t_hi) {                                                          // :174-189
                s.clock = SYNC_ADD(sync_filter_clamped(s, p, SYNC_SUB(t, p.sps)), p.sps);
                s.next_sym_middle = SYNC_ADD(s.last_sym_boundary_pos, SYNC_MUL(s.clock, 0.5f));
                while (s.next_sym_middle < s.stream_pos) s.next_sym_middle = SYNC_ADD(s.next_sym_middle, s.clock);
            }
        }
        s.last_sym_boundary_pos = s.stream_pos;
        s.last_sign = (int)sign;
    }
    s.stream_pos = SYNC_ADD(s.stream_pos, 1.0f);                                                     // :199-209
    const float step_back = SYNC_MUL(10.0f, s.clock);
    if (s.stream_pos > step_back && s.last_sym_boundary_pos > step_back && s.next_sym_middle > step_back) {
        s.stream_pos = SYNC_SUB(s.stream_pos, step_back);
        s.last_sym_boundary_pos = SYNC_SUB(s.last_sym_boundary_pos, step_back);
        s.next_sym_middle = SYNC_SUB(s.next_sym_middle, step_back);
    }
    return emit;
}

// Word w of a window of n samples: bit b = x[64 w + b] > 0.0 (NaN, +-0.0 and -Inf give 0, :154), 0 beyond the window.
inline unsigned long long sync_sign_word(const float* x, long n, long w) {
    unsigned long long m = 0;
    for (int b = 0; b < 64; ++b) {
        const long i = 64 * w + b;
        if (i < n && x[i] > 0.0f) m |= 1ull << b;
    }
    return m;
}
// The clock kernel's lane over one stream's window: the sign words in, per emission its window-relative index and clock value
// out (clk may be null), the count returned.
RR_SYNC_HD long sync_walk(SyncState& s, const SyncParams& p, const unsigned long long* words, long n, unsigned* idx, float* clk) {
    long k = 0;
    for (long i0 = 0; i0 < n; i0 += 64) {
        const unsigned long long m = words[i0 >> 6];
        const int lim = n - i0 < 64 ? (int)(n - i0) : 64;
        for (int b = 0; b < lim; ++b) {
            float c;
            if (sync_step(s, p, ((m >> b) & 1ull) != 0, &c)) {
                idx[k] = (unsigned)(i0 + b);
                if (clk) clk[k] = c;
                ++k;
            }
        }
    }
    return k;
}

}  // namespace rr
