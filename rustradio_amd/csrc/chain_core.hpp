// chain_core.hpp — the window bookkeeping of the fused chains on an FftFilter (FmChain, AudioChain, FmMulti, FmReceiver; DESIGN.md
// 4.2): plain integer functions, no HIP types, so tests/cpp/test_chain_hostlogic.cpp compiles them with g++.
//
// A chain runs whole filter blocks of S samples through FftFilter -> RationalResampler(I : D, reduced) [-> a demodulator that lags
// the resampler by `lag` samples].  After y filtered samples it has made resampled(y) = ceil(y I / D) samples and emitted
// max(resampled(y) - lag, 0).  `front` = L1 - 1 samples of a fused front FirFilter stay in the caller's window (fir.rs:537).
#pragma once
#include <cstdint>

namespace rr {

constexpr int CHAIN_WAIT_SRC = 1, CHAIN_WAIT_DST = 2;         // RR_WAIT_SRC, RR_WAIT_DST (include/rustradio_amd.h)

// S: the filter's block length (nsamples); I, D <= 2^31 each
struct ChainShape { uint64_t S; int64_t I, D; uint64_t lag, front; };
inline uint64_t chain_resampled(const ChainShape& c, uint64_t y) { return (uint64_t)(((__int128)y * c.I + c.D - 1) / c.D); }
inline uint64_t chain_lagged(const ChainShape& c, uint64_t r) { return r > c.lag ? r - c.lag : 0; }
inline uint64_t chain_emitted(const ChainShape& c, uint64_t y) { return chain_lagged(c, chain_resampled(c, y)); }
// outputs the next filter block adds behind n1 filtered samples
inline uint64_t chain_next_block_outputs(const ChainShape& c, uint64_t n1) { return chain_emitted(c, n1 + c.S) - chain_emitted(c, n1); }

// One call: k blocks run, `consumed` elements leave the window, new_pend stay pending, `produced` outputs appear, and the call
// answers status(need).  early: one of the two answers that come before anything is touched (k = consumed = produced = 0).
struct ChainPlan {
    int status; uint64_t need; bool early;
    uint64_t k, n_y, consumed, new_pend, produced;
    uint64_t o_old, r_lo, r_hi;   // the kernel's ranges: outputs emitted before the call, resampled(n1), resampled(n1 + n_y)
};
// n1 filtered samples so far, pend_len (< S) pending; the call offers in_len elements, room for out_cap outputs, max_blocks blocks.
// Like FftFilter::work (fft_filter.rs:294-326): room for one block's outputs first, then blocks while input and room last.
// A tie — the input's last full block is also the last that fits — answers WAIT_SRC here (k_in > k_out, not >=).  The bare
// FftFilter::work_dev (blocks.cpp) answers WAIT_DST(S) on its tie, k_in >= k_out: it follows the reference's loop, which looks at the
// output window before it reads (fft_filter.rs:292-304) and so leaves the rest of the input where it is, while the filter inside
// a chain writes to an inner stream and takes the rest in as pending samples.  That one stays outside this plan.
inline ChainPlan chain_plan(const ChainShape& c, uint64_t n1, uint64_t pend_len, uint64_t in_len, uint64_t out_cap, uint64_t max_blocks) {
    ChainPlan p{};
    p.new_pend = pend_len;
    p.r_lo = p.r_hi = chain_resampled(c, n1);
    p.o_old = chain_lagged(c, p.r_lo);
    p.early = true;
    const uint64_t need_next = chain_emitted(c, n1 + c.S) - p.o_old;
    if (need_next > out_cap) { p.status = CHAIN_WAIT_DST; p.need = need_next; return p; }
    if (c.front && in_len < c.front + 1) { p.status = CHAIN_WAIT_SRC; p.need = c.front + 1; return p; }   // fir.rs:498-501
    p.early = false;
    const uint64_t av = in_len - c.front, total = pend_len + av, k_in = total / c.S;
    // largest k with emitted(n1 + k S) - o_old <= out_cap  <=>  ceil((n1 + k S) I / D) <= o_old + out_cap + lag  <=>  n1 + k S <= X
    const __int128 X = (__int128)(p.o_old + out_cap + c.lag) * c.D / c.I;
    uint64_t k_out = X >= (__int128)n1 ? (uint64_t)((X - n1) / c.S) : 0;
    while (k_out > 0 && chain_emitted(c, n1 + k_out * c.S) - p.o_old > out_cap) k_out--;
    if (k_out > max_blocks) k_out = max_blocks;
    if (k_in > k_out) {
        p.k = k_out; p.consumed = p.k * c.S - pend_len; p.new_pend = 0;
        p.status = CHAIN_WAIT_DST; p.need = chain_next_block_outputs(c, n1 + p.k * c.S);
    } else {
        p.k = k_in; p.consumed = av; p.new_pend = total - p.k * c.S;
        p.status = CHAIN_WAIT_SRC; p.need = c.S - p.new_pend + c.front;
    }
    p.n_y = p.k * c.S;
    p.r_hi = chain_resampled(c, n1 + p.n_y);
    p.produced = chain_lagged(c, p.r_hi) - p.o_old;
    return p;
}

// ---- the N-station receiver: an RF chain `rf` into an audio chain `au` (lag 0) ----------------------------------------------------
// A(k): audio samples after k RF filter blocks — the audio stage filters whole blocks of the demodulated samples
inline uint64_t receiver_audio_after(const ChainShape& rf, const ChainShape& au, uint64_t k) {
    return chain_resampled(au, chain_emitted(rf, k * rf.S) / au.S * au.S);
}
// stage 2 of a call: p1 new demodulated samples behind pend_len carried ones, n1 audio-stage samples filtered so far
struct ReceiverSplit { uint64_t total, k2, n_y, new_pend, r_lo, r_hi; };
inline ReceiverSplit receiver_split(const ChainShape& au, uint64_t n1, uint64_t pend_len, uint64_t p1) {
    const uint64_t total = pend_len + p1, k2 = total / au.S, n_y = k2 * au.S;
    return ReceiverSplit{total, k2, n_y, total - n_y, chain_resampled(au, n1), chain_resampled(au, n1 + n_y)};
}

}  // namespace rr
