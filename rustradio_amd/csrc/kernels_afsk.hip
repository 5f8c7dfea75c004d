// kernels_afsk.hip — the tone demodulator of the 1200-baud receivers (examples/ax25-1200-rx.rs:238-247, il2p-1200-rx.rs:81-89),
//   Hilbert -> QuadratureDemod -> FftFilterFloat (as its definition, a direct sum) -> AddConst,
// over the next n samples of nstreams independent streams in ONE launch (the arithmetic and the indexing are
// afsk_core.hpp's).  blockIdx.y is the stream, blockIdx.x the tile of AFSK_TILE outputs; a workgroup reads its input window plus
// halo (L - 1 + H samples) once, recomputes the demodulated samples over the halo and keeps nothing for its neighbour, so no
// workgroup waits on another and there are no atomics.  The last tile of a stream also writes the stream's next carry into the
// OTHER buffer of the pair, which no workgroup of the launch reads.  The grid depends on n and nstreams alone.
#include "kernels.hpp"

namespace rr {

__global__ __launch_bounds__(AFSK_NT) void k_afsk(AfskArgs a) {
    extern __shared__ float afsk_lds[];
    float* X = afsk_lds;
    float* D = X + a.g.x_floats;
    float* HR = D + a.g.d_floats;
    const int tid = threadIdx.x;
    const long c = blockIdx.y, tx = blockIdx.x;
    afsk_load(a, c, tx, blockIdx.x == gridDim.x - 1, tid, X, D, HR);
    const int nk = afsk_tile_nk(a, tx), ng = afsk_tile_groups(a, nk);
    if (!nk) return;                                                   // (workgroup-uniform: only a push that produces nothing)
    __syncthreads();
    for (int g = tid; g < ng; g += AFSK_NT) afsk_demod(a, tx * AFSK_TILE, g, X, HR, D);
    __syncthreads();
    for (int j = tid; j < a.g.L; j += AFSK_NT) X[j] = a.taps[j];      // X is done with: the taps take its place
    __syncthreads();
    if (AFSK_R * tid >= nk) return;
    float y[AFSK_R];
    afsk_lowpass(a, tid, X, D, y);
    float* out = a.out + c * a.out_stride + tx * AFSK_TILE + AFSK_R * tid;
#pragma unroll
    for (int r = 0; r < AFSK_R; r++)
        if (AFSK_R * tid + r < nk) out[r] = y[r];
}

void launch_afsk(const AfskArgs& a, long nstreams, hipStream_t s) {
    if (a.n <= 0 || nstreams <= 0) return;
    const long ntiles = afsk_tiles(a.produced);
    hipLaunchKernelGGL(k_afsk, dim3((unsigned)ntiles, (unsigned)nstreams), dim3(AFSK_NT), (size_t)a.g.lds_floats * sizeof(float), s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
