// kernels_sync.hip — the symbol clock of the streaming data receivers (examples/ax25-9600-rx.rs:186-193, ax25-1200-rx.rs:293-300,
// il2p-1200-rx.rs:110-117):
//   SymbolSync (src/symbol_sync.rs:115-217) with TedZeroCrossing and IirFilter::filter_clamped (src/iir_filter.rs:104-125)
// over the next n samples of nstreams independent streams (the arithmetic is symsync_core.hpp's).  Sample values
// reach the state only through `sample > 0.0` and the emitted value is a copy, so a push is
//   k_sync_signs     every sample of every stream: x > 0.0 packed 64 to a word by wave ballot (window-relative words, the last
//                    partial one zero-filled)
//   k_sync_clock     one lane per stream: the carried state, the reference's loop sample by sample over the sign words; per
//                    emission its window-relative index and the clock value, the count, the new state
//   k_sync_gather    syms[c][k] = in[c][idx[c][k]], k < count[c] (the count is read on the device)
// The filter never forgets and every f32 operation is rounded on its own, so there is no parallel form within a stream: the
// streams are the parallelism.  No lane waits on another; there are no atomics.  The grids depend on n and nstreams alone.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
constexpr int SY_B = 256;                     // threads of a workgroup of k_sync_signs / k_sync_gather

__global__ __launch_bounds__(SY_B) void k_sync_signs(SyncArgs a) {
    const int lane = threadIdx.x & 63;
    const long total = a.nstreams * a.nwords, step = (long)gridDim.x * (SY_B / 64);
    for (long g = (long)blockIdx.x * (SY_B / 64) + (threadIdx.x >> 6); g < total; g += step) {      // (wave-uniform)
        const long c = g / a.nwords, w = g - c * a.nwords, i = (w << 6) + lane;
        const float x = i < a.n ? a.in[c * a.in_stride + i] : 0.0f;
        const u64 m = __ballot(x > 0.0f);
        if (lane == 0) a.words[g] = m;
    }
}

// One wave per workgroup.  spw == 1: stream blockIdx.x on lane 0, the other lanes idle.  spw == 64: stream 64 blockIdx.x + lane.
__global__ __launch_bounds__(64) void k_sync_clock(SyncArgs a) {
    const long c = a.spw == 1 ? (threadIdx.x == 0 ? (long)blockIdx.x : a.nstreams) : (long)blockIdx.x * 64 + threadIdx.x;
    if (c >= a.nstreams) return;
    SyncState st = a.st_in[c];
    const long k = sync_walk(st, a.prm, a.words + c * a.nwords, a.n, a.idx + c * a.n, a.clk ? a.clk + c * a.out_stride : nullptr);
    a.count[c] = (u64)k;
    a.st_out[c] = st;
}

// blockIdx.y: the stream; the workgroups of a row stride over its emissions
__global__ __launch_bounds__(SY_B) void k_sync_gather(SyncArgs a) {
    const long c = blockIdx.y;
    const u64 cnt = a.count[c];
    const long kmax = cnt < (u64)a.n ? (long)cnt : a.n;
    const float* in = a.in + c * a.in_stride;
    const unsigned* idx = a.idx + c * a.n;
    float* out = a.syms + c * a.out_stride;
    for (long k = (long)blockIdx.x * SY_B + threadIdx.x; k < kmax; k += (long)gridDim.x * SY_B) {
        const long j = idx[k];
        if (j < a.n) out[k] = in[j];
    }
}

void launch_sync(const SyncArgs& a, int which, hipStream_t s) {
    if (a.n <= 0 || a.nstreams <= 0) return;
    if (which == 0 || which == 1)
        hipLaunchKernelGGL(k_sync_signs, dim3(tiles_grid((a.nstreams * a.nwords + SY_B / 64 - 1) / (SY_B / 64))), dim3(SY_B), 0, s, a);
    if (which == 0 || which == 2)
        hipLaunchKernelGGL(k_sync_clock, dim3((unsigned)(a.spw == 1 ? a.nstreams : (a.nstreams + 63) / 64)), dim3(64), 0, s, a);
    if (which == 0 || which == 3) {
        const long per_row = std::max<long>(1, std::min<long>((a.n + SY_B - 1) / SY_B, std::max<long>(1, (long)device_cu_count() * 8 / a.nstreams)));
        hipLaunchKernelGGL(k_sync_gather, dim3((unsigned)per_row, (unsigned)a.nstreams), dim3(SY_B), 0, s, a);
    }
    RR_HIP(hipGetLastError());
}

}  // namespace rr
