// kernels_saver.hip — Delay (src/delay.rs:62-111) and the data branch of examples/burst_saver.rs:111-131: Delay(3000) in front of
// StreamToPdu<Complex>.
//
// Delay over one work() call is a fill and a copy: out[i] = 0 for i < zeros, in[i - zeros] behind them.  The counts depend on
// lengths alone (saver_host.hpp delay_step), so nothing is carried on the device.
//
// The burst saver's data branch writes what k_pdu_tiles<false> writes for an f32 handle — the window behind the open burst in
// the arena — with the window taken `delay` samples late: the first min(n, delay) samples come from the history (the last
// `delay` input samples, zeros in front of the stream), the rest from the window itself; the next history is the old one
// moved down by n with the window's last samples behind it.  hist_in / hist_out are distinct buffers (the block's ping-pong),
// so no thread reads what another one writes.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

constexpr int SAVER_B = 256;

template <class T> __global__ __launch_bounds__(SAVER_B) void k_delay(const T* __restrict__ in, T* __restrict__ out, long zeros, long total) {
    for (long i = (long)blockIdx.x * SAVER_B + threadIdx.x; i < total; i += (long)gridDim.x * SAVER_B) out[i] = i < zeros ? T(0) : in[i - zeros];
}
void launch_delay(const void* in, void* out, long zeros, long copied, size_t es, hipStream_t s) {
    const long total = zeros + copied;
    if (total <= 0) return;
    const unsigned grid = tiles_grid((total + SAVER_B - 1) / SAVER_B);
    if (es == 1)
        hipLaunchKernelGGL((k_delay<unsigned char>), dim3(grid), dim3(SAVER_B), 0, s, static_cast<const unsigned char*>(in),
                           static_cast<unsigned char*>(out), zeros, total);
    else if (es == 4)
        hipLaunchKernelGGL((k_delay<unsigned>), dim3(grid), dim3(SAVER_B), 0, s, static_cast<const unsigned*>(in), static_cast<unsigned*>(out),
                           zeros, total);
    else
        hipLaunchKernelGGL((k_delay<unsigned long long>), dim3(grid), dim3(SAVER_B), 0, s, static_cast<const unsigned long long*>(in),
                           static_cast<unsigned long long*>(out), zeros, total);
    RR_HIP(hipGetLastError());
}

// Complex samples move as 64-bit words (SaverArgs): every payload bit survives, NaN payloads included
__global__ __launch_bounds__(SAVER_B) void k_saver_copy(SaverArgs a) {
    const long t0 = (long)blockIdx.x * SAVER_B + threadIdx.x, step = (long)gridDim.x * SAVER_B;
    // the open burst: its samples so far end the previous arena; they go in front of arena[C) (as in k_pdu_tiles)
    const unsigned long long orr = a.st_in->open_r;
    long clen = (orr == PDU_NONE || !a.prev_arena) ? 0 : (long)(a.w0 - orr);
    clen = clen < a.C ? clen : a.C;
    for (long k = t0; k < clen; k += step) {
        const long idx = a.C - clen + k;
        a.arena[idx] = a.prev_arena[idx + a.n_prev];
    }
    // the delayed window
    for (long i = t0; i < a.n; i += step) a.arena[a.C + i] = i < a.from_hist ? a.hist_in[i] : a.x[i - a.delay];
    // the last `delay` input samples after this window
    for (long j = t0; j < a.delay; j += step) a.hist_out[j] = j < a.shifted ? a.hist_in[j + a.n] : a.x[j + a.n - a.delay];
}
void launch_saver_copy(const SaverArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    const long most = std::max(std::max(a.n, a.delay), a.C);
    hipLaunchKernelGGL(k_saver_copy, dim3(tiles_grid((most + SAVER_B - 1) / SAVER_B)), dim3(SAVER_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
