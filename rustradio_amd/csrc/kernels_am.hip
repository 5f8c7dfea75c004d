// kernels_am.hip — the audio path of examples/airspy_am_decode.rs,
//   Map(|v| v.norm()) -> FftFilterFloat (as its definition, a direct sum) -> RationalResampler -> MultiplyConst,
// over the next n Complex samples of nstreams independent streams in ONE launch (the arithmetic and the indexing
// are am_core.hpp's).  blockIdx.y is the stream, blockIdx.x the tile of a.g.T outputs.  Only the filter outputs the resampler
// picks are summed.  A workgroup stages the magnitudes of its outputs' windows itself, chunk of taps by chunk, and keeps nothing
// for its neighbour, so no workgroup waits on another and there are no atomics.  The last tile of a stream also writes the
// stream's next carry into the OTHER buffer of the pair, which no workgroup of the launch reads.  The grid depends on the
// lengths and nstreams alone.
#include "kernels.hpp"

namespace rr {

__global__ __launch_bounds__(AM_NT) void k_am(AmArgs a) {
    extern __shared__ float am_lds[];
    float* S = am_lds;
    int* B = reinterpret_cast<int*>(am_lds + AM_LDS_FLOATS);           // S index of term j0 of each output of the tile
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long c = blockIdx.y, tx = blockIdx.x;
    if (blockIdx.x == gridDim.x - 1) am_carry(a, c, tid);
    const int nk = am_tile_nk(a, tx);
    if (!nk) return;                                                   // (workgroup-uniform: only a push that produces nothing)
    if (tid < a.g.T) B[tid] = am_base(a, tx, tid < nk ? tid : nk - 1);
    __syncthreads();
    float acc[AM_NG_MAX][AM_G];
    int base[AM_NG_MAX][AM_G];
#pragma unroll
    for (int g = 0; g < AM_NG_MAX; g++)
#pragma unroll
        for (int u = 0; u < AM_G; u++) {
            acc[g][u] = 0.0f;
            base[g][u] = g < a.g.NG ? B[(AM_WAVES * g + w) * AM_G + u] : 0;
        }
    for (int j0 = 0; j0 < a.g.L; j0 += a.g.KC) {
        if (j0) __syncthreads();                                       // the chunk before has been read
        am_stage(a, c, tx, nk, j0, tid, S);
        __syncthreads();
#pragma unroll
        for (int g = 0; g < AM_NG_MAX; g++)
            if (g < a.g.NG && (AM_WAVES * g + w) * AM_G < nk) am_accum(a, j0, lane, base[g], S, acc[g]);
    }
    float* out = a.out + c * a.out_stride + tx * a.g.T;
#pragma unroll
    for (int g = 0; g < AM_NG_MAX; g++) {
        const int r0 = (AM_WAVES * g + w) * AM_G;
        if (g >= a.g.NG || r0 >= nk) continue;                         // (wave-uniform)
        float mine = 0.0f;
#pragma unroll
        for (int u = 0; u < AM_G; u++) {
            float y = acc[g][u];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) y = AM_ADD(y, __shfl_xor(y, d));
            if (lane == u) mine = y;
        }
        if (lane < AM_G && r0 + lane < nk) out[r0 + lane] = am_scale(a, mine);
    }
}

size_t am_lds_bytes() { return (size_t)AM_LDS_FLOATS * sizeof(float) + (size_t)(32 * AM_NG_MAX) * sizeof(int); }

void launch_am(const AmArgs& a, long nstreams, hipStream_t s) {
    if (a.n <= 0 || nstreams <= 0) return;
    const long ntiles = am_tiles(a.g, a.produced);
    hipLaunchKernelGGL(k_am, dim3((unsigned)ntiles, (unsigned)nstreams), dim3(AM_NT), am_lds_bytes(), s, a);
    RR_HIP(hipGetLastError());
}

// ---- AirSPY samples (examples/airspy_am_decode.rs: Map "AirSPY to Complex"): little-endian u32, I in the low 16 bits and Q in the
// high 16, each an i16 -> Complex(f32(i) / 1000, f32(q) / 1000).  Two true f32 divisions (num-complex divides each component):
// bit-exact.  12 B of traffic per sample, lane-consecutive.
__global__ __launch_bounds__(256) void k_airspy_decode(const unsigned* __restrict__ in, cf* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const unsigned v = in[i];
        out[i] = mkcf((float)(short)(v & 0xffffu) / 1000.0f, (float)(short)(v >> 16) / 1000.0f);
    }
}
void launch_airspy_decode(const unsigned* in, cf* out, long n, hipStream_t s) {
    if (n <= 0) return;
    const long blocks = std::min<long>((n + 255) / 256, (long)device_cu_count() * 16);
    hipLaunchKernelGGL(k_airspy_decode, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
