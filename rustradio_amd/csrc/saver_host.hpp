// saver_host.hpp — the host-only logic of Delay (src/delay.rs:62-111) and of the burst saver (examples/burst_saver.rs): what is
// refused, what one work() call of Delay moves, and where the samples of a push come from (the window or the history).  No HIP
// in here, so tests/cpp/test_saver_hostlogic.cpp builds it with the host sanitizers and drives it without a device.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/rustradio_amd.h"
#include "pdu_host.hpp"

namespace rr {

constexpr size_t DELAY_MAX = 1024000;         // the cap of a push in this family (a deviation: the reference takes any usize)
constexpr size_t SAVER_MAX_WINDOW = 1024000;

// What rr_delay_create refuses, said before any device is touched; nullptr: fine.
inline const char* delay_check(size_t delay, size_t elem_size) {
    if (elem_size != 1 && elem_size != 4 && elem_size != 8) return "unsupported element size";
    if (delay > DELAY_MAX) return "delay: more than 1,024,000 samples";
    return nullptr;
}
// ... and rr_burst_saver_create (the detector's, StreamToPdu's and Delay's refusals, in that order)
inline const char* saver_check(float alpha, size_t delay, size_t max_size) {
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return "alpha out of range";
    if (const char* e = pdu_check(max_size, 0)) return e;
    return delay_check(delay, 8);
}
// ... and a push of it
inline const char* saver_push_check(const void* in, size_t n) {
    if (n > SAVER_MAX_WINDOW) return "window longer than 1024000 samples";
    if (n && !in) return "null argument";
    return nullptr;
}

// One work() call of Delay: the loop of delay.rs:64-110 with no skip pending.  `zeros` default elements, then `copied` input
// samples; `remaining` is current_delay and is updated.  Depends on lengths only.
struct DelayStep {
    size_t zeros, copied;
    int status;                               // RR_WAIT_DST: no output space left (:80-82); RR_WAIT_SRC: no input left (:94-96)
};
inline DelayStep delay_step(size_t& remaining, size_t in_len, size_t out_cap) {
    DelayStep d{0, 0, RR_WAIT_DST};
    if (out_cap == 0) return d;
    d.zeros = std::min(remaining, out_cap);
    remaining -= d.zeros;
    size_t room = out_cap - d.zeros;
    if (room == 0) return d;
    d.copied = std::min(in_len, room);
    room -= d.copied;
    d.status = room == 0 ? RR_WAIT_DST : RR_WAIT_SRC;         // the loop's next turn tests the output first
    return d;
}

// Where a push of n samples takes the delayed stream from, with `hist` the last `delay` input samples (zeros in front of the
// stream): delayed[i] = i < from_hist ? hist[i] : x[i - delay], and the next history is
// next[j] = j < shifted ? hist[j + n] : x[j + n - delay].  A push shorter than the delay shifts the history and appends.
struct SaverPlan {
    size_t from_hist;                         // samples of the delayed window the history supplies: min(n, delay)
    size_t shifted;                           // entries of the next history that are old ones moved down: delay - min(n, delay)
};
inline SaverPlan saver_plan(size_t n, size_t delay) {
    const size_t k = std::min(n, delay);
    return SaverPlan{k, delay - k};
}

// launches of one push of n > 0 samples: the envelope (1, or 3 beyond one tile), the delayed copy, StreamToPdu's closed form
inline size_t saver_launches(size_t n, size_t iir_tile) {
    if (!n) return 0;
    size_t k = 0;
    for (const size_t maxr = n / 2 + 1; ((size_t)1 << k) < maxr; ++k) {}
    return (n <= iir_tile ? 1 : 3) + 1 + 5 + k;
}

}  // namespace rr
