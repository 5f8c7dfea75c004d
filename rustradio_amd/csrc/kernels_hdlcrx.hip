// kernels_hdlcrx.hip — the end of the packet receivers (examples/ax25-9600-rx.rs:195-215, ax25-1200-rx.rs, bell202.rs) for N streams:
//   BinarySlicer (src/binary_slicer.rs:17-19) -> XorConst(1) -> NrziDecode (src/nrzi.rs:36-41) -> Descrambler
//   (src/descrambler.rs:34-39) -> HdlcDeframer (src/hdlc_deframer.rs:123-232)
// over the ragged symbol windows rr_symbol_sync leaves on the device.  The seven launches of kernels_hdlc.hip and
// their bodies (hdlc_body.hpp), with the stream as the grid's y:
//   k_rx_mark        as k_hdlc_mark, but the tile's words come from f32 symbols: sign words by ballot, then the inversion, NRZI
//                    and the descrambler as shifts and XORs on words (hdlcrx_core.hpp) — no byte-per-bit stream exists
//   k_rx_offs / _resolve / _carry    one workgroup per STREAM
//   k_rx_ends / _gap / _emit         workgroups (x, stream) stride over that stream's own tiles, gaps and frames, whose numbers they
//                    read on the device; a workgroup with nothing to do leaves at once
// Every kernel builds stream blockIdx.y's view from base pointers and pitches (rx_view); its symbol count is read there and
// clamped to n_cap.  No workgroup waits on another; the grids depend on nstreams, n_cap and the host's bound of the carry alone.
// Who resets what: each stream has its own three push counters (pstats), zeroed by that stream's first mark workgroup; the record
// list and its counter are shared by all streams, and the first mark workgroup of stream 0 zeroes the counter.  Both are added to
// only by k_rx_emit, four launches later.  Each stream owns p_arena bytes of the arena, so every arena byte still has one writer.
#include "hdlc_body.hpp"
#include "hdlcrx_core.hpp"

namespace rr {

static_assert(sizeof(HdlcRxRec) == 32, "HdlcRxRec is rr_hdlc_stream_frame");
constexpr int RX_HW = 2;                      // words of history in front of a tile
constexpr int RX_NW = RX_HW + HD_W;

__device__ __forceinline__ HdlcArgs rx_view(const HdlcRxArgs& r, long c) {
    HdlcArgs a = r.h;
    const u64 k = r.counts ? r.counts[c] : (u64)r.n_cap;
    a.n = k < (u64)r.n_cap ? (long)k : r.n_cap;                  // the device's count is clamped before anything uses it
    a.cin += c * r.p_carry; a.cout += c * r.p_carry;
    a.st_in += c; a.st_out += c;
    a.w0 = r.bst_in[c * RX_ST_N + RX_ST_POS];
    a.raw += c * r.p_words; a.fl += c * r.p_words; a.ab += c * r.p_words; a.sf += c * r.p_words;
    a.tilecnt += c * r.p_tiles; a.offs += c * r.p_tiles;
    a.etotal += c; a.fin += c; a.pstats += 3 * c;
    a.ends += c * r.p_ends; a.gmap += c * r.p_ends; a.pmap += c * r.p_ends;
    a.bmap += c * r.p_blocks; a.bstate += c * r.p_blocks;
    a.arena += c * r.p_arena;
    // the stream's own tiles, at most the host's: a stream with no symbols has none, so it has no flag ends and emits nothing
    const long nt = a.n ? (hd_nv(a) + HDLC_T - 1) / HDLC_T : 0;
    a.ntiles = nt < r.h.ntiles ? nt : r.h.ntiles;
    return a;
}

// The symbol source of one stream: see hdlcrx_core.hpp for the coordinates.
struct HdlcRxSrc {
    const float* x;                           // the stream's symbols
    bool invert, nrzi;
    u64 dmask, rlast, dhist;
    u64* st_out;                              // the stream's RX_ST_N words
    // r at virtual position v (binary_slicer.rs:17-19: NaN, -0.0 -> 0)
    __device__ __forceinline__ bool rbit(long C, long nv, long v) const {
        if (v >= C) return v < nv && (x[v - C] > 0.0f) != invert;
        return v == C - 1 && rlast != 0;
    }
    __device__ __forceinline__ void fill(const HdlcArgs& a, long C, long nv, long t0, u64* s_raw, u64* s_prev) const {
        __shared__ u64 s_r[RX_NW], s_d[RX_NW], s_c[HD_W];
        __shared__ u64 s_s1;
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const bool carried = t0 < C;          // (uniform) the tile holds bits the previous push left, already decoded
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long v = t0 + i * HD_B + tid;
            const u64 b = __ballot(rbit(C, nv, v));
            if (lane == 0) s_r[RX_HW + i * (HD_B / 64) + wave] = b;
            if (carried) {
                const u64 cb = __ballot(v < C && (a.cin[v] & 1u) != 0);
                if (lane == 0) s_c[i * (HD_B / 64) + wave] = cb;
            }
        }
        if (wave < RX_HW) {                   // the 128 positions in front of the tile
            const u64 b = __ballot(rbit(C, nv, t0 - 64 * RX_HW + tid));
            if (lane == 0) s_r[wave] = b;
        }
        __syncthreads();
        if (tid < RX_NW) {
            const long vb = t0 - 64 * RX_HW + 64 * tid;
            s_d[tid] = rx_patch_d(rx_nrzi_word(s_r[tid], tid ? s_r[tid - 1] : 0ull, nrzi), vb, C, dhist);
        }
        __syncthreads();
        if (tid >= 1 && tid < RX_NW) {        // (word 0 of S is never looked at)
            const long vb = t0 - 64 * RX_HW + 64 * tid;
            const u64 s = rx_descramble_word(s_d[tid], s_d[tid - 1], dmask);
            if (tid >= RX_HW) s_raw[tid - RX_HW] = rx_final_word(s, carried ? s_c[tid - RX_HW] : 0ull, vb, C, nv);
            else s_s1 = rx_final_word(s, 0ull, vb, C, nv);
        }
        // the thread that holds the push's last symbol writes what the bit chain of the next push starts from
        if (tid == HD_B - 1 && nv > C && nv - 1 >= t0 && nv - 1 < t0 + HDLC_T) {
            const long p = nv - 1 - (t0 - 64 * RX_HW);
            st_out[RX_ST_RLAST] = s_r[p >> 6] >> (p & 63) & 1ull;
            st_out[RX_ST_DHIST] = rx_win64(s_d, p);
            st_out[RX_ST_POS] = a.w0 + (u64)(nv - C);
        }
        __syncthreads();
        if (wave == 0) {                      // the 8 bits in front of the tile
            const long v = t0 - 8 + lane;
            const bool bit = lane < 8 && v >= 0 && (v < C ? (a.cin[v] & 1u) != 0 : (s_s1 >> (v & 63) & 1ull) != 0);
            const u64 h = __ballot(bit);
            if (lane == 0) *s_prev = h << 56;
        }
        __syncthreads();
    }
};
struct HdlcRxSink {
    HdlcRxRec* recs;
    unsigned stream;
    u64 start0;                               // where the stream's region of the arena begins
    __device__ __forceinline__ void record(const HdlcArgs& a, u64 pos, u64 start, unsigned len, unsigned flags) const {
        const u64 slot = atomicAdd(a.count, 1ull);
        if (slot < (u64)a.rec_cap) recs[slot] = HdlcRxRec{pos, start0 + start, len, flags, stream, 0u};
    }
};

__global__ __launch_bounds__(HD_B) void k_rx_mark(HdlcRxArgs r) {
    const long c = blockIdx.y;
    const HdlcArgs a = rx_view(r, c);
    const u64* bi = r.bst_in + c * RX_ST_N;
    u64* bo = r.bst_out + c * RX_ST_N;
    if (a.n == 0 && blockIdx.x == 0 && threadIdx.x < RX_ST_N) bo[threadIdx.x] = bi[threadIdx.x];      // nothing moves: the state is kept
    const HdlcRxSrc src{r.syms + c * r.stride, r.invert != 0, r.nrzi != 0, r.dmask, bi[RX_ST_RLAST], bi[RX_ST_DHIST], bo};
    hd_mark_body(a, src, blockIdx.x == 0 && c == 0, blockIdx.x == 0);
}
__global__ __launch_bounds__(HD_SB) void k_rx_offs(HdlcRxArgs r) { hd_offs_body(rx_view(r, blockIdx.y)); }
__global__ __launch_bounds__(64) void k_rx_ends(HdlcRxArgs r) { hd_ends_body(rx_view(r, blockIdx.y)); }
__global__ __launch_bounds__(HDLC_GB) void k_rx_gap(HdlcRxArgs r) { hd_gap_body(rx_view(r, blockIdx.y)); }
__global__ __launch_bounds__(HD_SB) void k_rx_resolve(HdlcRxArgs r) { hd_resolve_body(rx_view(r, blockIdx.y)); }
__global__ __launch_bounds__(HD_B) void k_rx_emit(HdlcRxArgs r) {
    const long c = blockIdx.y;
    hd_emit_body(rx_view(r, c), HdlcRxSink{r.recs, (unsigned)c, (u64)c * (u64)r.p_arena});
}
__global__ __launch_bounds__(HD_B) void k_rx_carry(HdlcRxArgs r) {
    const HdlcArgs a = rx_view(r, blockIdx.y);
    if (a.n == 0) {                           // nothing moved: every piece of the state goes to the buffers the next push reads
        const long C = hd_carried(a);
        for (long i = threadIdx.x; i < C; i += HD_B) a.cout[i] = a.cin[i];
        if (threadIdx.x == 0) *a.st_out = *a.st_in;
        return;
    }
    hd_carry_body(a);
}

// x workgroups per stream for `per_stream` pieces of work each: all of them while the device has room, else a share of eight per CU
static unsigned rx_grid_x(long per_stream, long nstreams) {
    const long room = ((long)device_cu_count() * 8 + nstreams - 1) / nstreams;
    return (unsigned)std::max<long>(1, std::min(per_stream, room));
}

void launch_hdlcrx(const HdlcRxArgs& r, hipStream_t s) {
    if (r.n_cap <= 0 || r.nstreams <= 0) return;
    const unsigned ns = (unsigned)r.nstreams;
    const unsigned gt = rx_grid_x(r.h.ntiles, r.nstreams);
    const unsigned gg = rx_grid_x((r.h.ends_cap + HDLC_GB - 1) / HDLC_GB, r.nstreams);
    const unsigned ge = rx_grid_x((r.h.ends_cap + HD_B / 64 - 1) / (HD_B / 64), r.nstreams);
    hipLaunchKernelGGL(k_rx_mark, dim3(gt, ns), dim3(HD_B), 0, s, r);
    hipLaunchKernelGGL(k_rx_offs, dim3(1, ns), dim3(HD_SB), 0, s, r);
    hipLaunchKernelGGL(k_rx_ends, dim3(gt, ns), dim3(64), 0, s, r);
    hipLaunchKernelGGL(k_rx_gap, dim3(gg, ns), dim3(HDLC_GB), 0, s, r);
    hipLaunchKernelGGL(k_rx_resolve, dim3(1, ns), dim3(HD_SB), 0, s, r);
    hipLaunchKernelGGL(k_rx_emit, dim3(ge, ns), dim3(HD_B), 0, s, r);
    hipLaunchKernelGGL(k_rx_carry, dim3(1, ns), dim3(HD_B), 0, s, r);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
