// kernels_il2p.hip — the end of examples/il2p-1200-rx.rs:118-137 for N streams:
//   BinarySlicer (src/binary_slicer.rs:17-19) -> XorConst(1) -> CorrelateAccessCodeTag(SYNC_WORD, "sync", allowed_diffs)
//   (src/correlate_access_code.rs:93-118) -> Il2pDeframer (src/il2p_deframer.rs:172-237, 247-319)
// over the ragged symbol windows rr_symbol_sync leaves on the device.  Three launches, the stream as the grid's y:
//   k_il2p_mark   workgroups (x, stream) stride over the stream's tiles of IL2P_T symbols: sign words by ballot, the inversion, the
//                 match words (24 shifted XNOR terms for allowed_diffs == 0, a popcount per position otherwise) and the tile's map
//                 from the 121 entry states to its exit state, one lane per entry state
//   k_il2p_scan   one workgroup per STREAM composes its tiles' maps in order (16 chunks side by side, then the chunks in order),
//                 leaves every tile's entry state, and writes the stream's state for the next push
//   k_il2p_emit   one wave per tile walks the tile's accepted tags from its entry state; each lane takes one tag whose header
//                 ends inside the push, descrambles, packs, parses and writes the record
// No workgroup waits on another; the grids depend on nstreams and n_cap alone.  Who writes what: a tile's words of bits / mw / maps
// and its entry byte have one writer each (the tile's mark workgroup, the stream's scan workgroup); the record list and its counter
// are shared by all streams, zeroed by the caller and added to only by k_il2p_emit; stats are only ever added to.
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
static_assert(sizeof(Il2pRec) == 64, "Il2pRec is rr_il2p_header");
constexpr int IL2P_B = 256;                   // threads of a mark workgroup: 4 words per round of ballots
constexpr int IL2P_SB = 1024;                 // ... of a scan workgroup: 16 waves, one chunk of tiles each
constexpr int IL2P_SW = IL2P_SB / 64;

struct Il2pView {
    long n, nt;                               // the stream's symbols of this push and its tiles
    const float* x;
    const u64* si;
    u64* so;
    u64 *bits, *mw;
    unsigned char *maps, *entry;
    u64 pos0, seen0;
    int blocked0;
};
__device__ __forceinline__ Il2pView il2p_view(const Il2pArgs& a, long c) {
    Il2pView v;
    const u64 k = a.counts ? a.counts[c] : (u64)a.n_cap;
    v.n = k < (u64)a.n_cap ? (long)k : a.n_cap;                   // the device's count is clamped before anything uses it
    const long nt = (v.n + IL2P_T - 1) / IL2P_T;
    v.nt = nt < a.ntiles ? nt : a.ntiles;
    v.x = a.syms + c * a.stride;
    v.si = a.st_in + c * IL2P_ST_N;
    v.so = a.st_out + c * IL2P_ST_N;
    v.bits = a.bits + c * a.p_words;
    v.mw = a.mw + c * a.ntiles * IL2P_TW;
    v.maps = a.maps + c * a.ntiles * IL2P_MAP_PITCH;
    v.entry = a.entry + c * a.ntiles;
    v.pos0 = v.si[IL2P_ST_POS];
    const u64 sn = v.si[IL2P_ST_SEEN], bl = v.si[IL2P_ST_BLOCKED];
    v.seen0 = sn < 24 ? sn : 24;
    v.blocked0 = bl < (u64)IL2P_HEADER_BITS ? (int)bl : IL2P_HEADER_BITS;
    return v;
}

__global__ __launch_bounds__(IL2P_B) void k_il2p_mark(Il2pArgs a) {
    __shared__ u64 s_w[1 + IL2P_TW];          // [0]: the word in front of the tile
    __shared__ u64 s_m[IL2P_TW];
    const long c = blockIdx.y;
    const Il2pView v = il2p_view(a, c);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool inv = a.invert != 0;
    const long nv = IL2P_CARRY + v.n, first = il2p_first_valid(v.seen0);
    for (long t = blockIdx.x; t < v.nt; t += gridDim.x) {
        const long i0 = t * IL2P_T;
#pragma unroll
        for (int i = 0; i < IL2P_T / IL2P_B; ++i) {
            const long idx = i0 + i * IL2P_B + tid;
            // binary_slicer.rs:17-19: NaN, +-0.0 and -Inf slice to 0, then the inversion; nothing at or beyond the count is read
            const u64 b = __ballot(idx < v.n && (v.x[idx] > 0.0f) != inv);
            if (lane == 0) s_w[1 + i * (IL2P_B / 64) + wave] = b;
        }
        if (wave == 0) {
            if (t > 0) {                      // (the tile exists, so the 64 symbols in front of it do)
                const u64 b = __ballot((v.x[i0 - 64 + lane] > 0.0f) != inv);
                if (lane == 0) s_w[0] = b;
            } else if (lane == 0) s_w[0] = v.si[IL2P_ST_BITS + IL2P_CARRY_WORDS - 1];
        }
        __syncthreads();
        if (tid < IL2P_TW) v.bits[IL2P_CARRY_WORDS + t * IL2P_TW + tid] = s_w[1 + tid];
        if (t == 0 && tid >= 64 && tid < 64 + IL2P_CARRY_WORDS) v.bits[tid - 64] = v.si[IL2P_ST_BITS + tid - 64];
        if (t == v.nt - 1 && tid == 128) v.bits[IL2P_CARRY_WORDS + v.nt * IL2P_TW] = 0ull;     // the word a header's window may touch
        if (a.allowed == 0 || a.allowed >= (unsigned)IL2P_SYNC_BITS) {
            if (tid < IL2P_TW) s_m[tid] = il2p_match_word(s_w[1 + tid], s_w[tid], a.allowed, IL2P_CARRY + i0 + 64 * tid, first, nv);
        } else {
#pragma unroll 4
            for (int i = 0; i < IL2P_T / IL2P_B; ++i) {
                const int wj = i * (IL2P_B / 64) + wave;
                const long vb = IL2P_CARRY + i0 + 64 * wj;
                const u64 b = __ballot((unsigned)il2p_diffs_at(s_w[1 + wj], s_w[wj], lane) <= a.allowed);
                if (lane == 0) s_m[wj] = b & ~il2p_below(vb, first) & il2p_below(vb, nv);
            }
        }
        __syncthreads();
        const long len = v.n - i0 < IL2P_T ? v.n - i0 : IL2P_T;
        if (wave == 0) {
            const u64 m = s_m[lane];
            v.mw[t * IL2P_TW + lane] = m;
            int cnt = il2p_popc(m);
#pragma unroll
            for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0 && cnt) atomicAdd(a.stats + 2 * c + 1, (u64)cnt);
        } else if (tid - 64 < IL2P_STATES) {
            v.maps[t * IL2P_MAP_PITCH + tid - 64] = (unsigned char)il2p_tile_exit(s_m, len, tid - 64);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(IL2P_SB) void k_il2p_scan(Il2pArgs a) {
    __shared__ unsigned char s_comp[IL2P_SW][IL2P_MAP_PITCH];
    __shared__ int s_entry[IL2P_SW];
    __shared__ int s_exit;
    const Il2pView v = il2p_view(a, blockIdx.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (v.n == 0) {                           // nothing moves: every piece of the state is kept
        if (tid < IL2P_ST_N) v.so[tid] = v.si[tid];
        return;
    }
    const long chunk = (v.nt + IL2P_SW - 1) / IL2P_SW;
    const long t0 = wave * chunk < v.nt ? wave * chunk : v.nt, t1 = t0 + chunk < v.nt ? t0 + chunk : v.nt;
    int e0 = lane, e1 = lane + 64 < IL2P_STATES ? lane + 64 : 0;
    for (long t = t0; t < t1; ++t) {
        const unsigned char* mp = v.maps + t * IL2P_MAP_PITCH;
        e0 = mp[e0];
        e1 = mp[e1];
    }
    s_comp[wave][lane] = (unsigned char)e0;
    s_comp[wave][lane + 64] = (unsigned char)e1;
    __syncthreads();
    if (tid == 0) {
        int e = v.blocked0;
        for (int w = 0; w < IL2P_SW; ++w) {
            s_entry[w] = e;
            e = s_comp[w][e];
        }
        s_exit = e;
    }
    __syncthreads();
    if (lane == 0) {
        int e = s_entry[wave];
        for (long t = t0; t < t1; ++t) {
            v.entry[t] = (unsigned char)e;
            e = v.maps[t * IL2P_MAP_PITCH + e];
        }
    }
    if (tid == 0) {
        const u64 sn = v.seen0 + (u64)v.n;
        v.so[IL2P_ST_POS] = v.pos0 + (u64)v.n;
        v.so[IL2P_ST_SEEN] = sn < 24 ? sn : 24;
        v.so[IL2P_ST_BLOCKED] = (u64)s_exit;
    }
    if (tid < IL2P_CARRY_WORDS) v.so[IL2P_ST_BITS + tid] = il2p_win(v.bits, v.n + 64 * tid);   // the last IL2P_CARRY bits
    if (tid >= IL2P_ST_BITS + IL2P_CARRY_WORDS && tid < IL2P_ST_N) v.so[tid] = 0ull;
}

__global__ __launch_bounds__(64) void k_il2p_emit(Il2pArgs a) {
    __shared__ u64 s_m[IL2P_TW];
    const long c = blockIdx.y;
    const Il2pView v = il2p_view(a, c);
    const int lane = threadIdx.x;
    for (long t = blockIdx.x; t < v.nt; t += gridDim.x) {
        const long i0 = t * IL2P_T;
        const long len = v.n - i0 < IL2P_T ? v.n - i0 : IL2P_T;
        s_m[lane] = v.mw[t * IL2P_TW + lane];
        __syncthreads();
        // the walk is the same in every lane; lane k keeps the k-th tag (a tile has at most 34 of its own and the carried one)
        int cnt = 0;
        long mine = 0;
        bool have = false;
        if (t == 0 && v.blocked0 > 0) {       // the header the stream so far left open: its tag lies in front of the push
            if (lane == 0) { mine = (long)v.blocked0 - IL2P_STATES; have = true; }
            cnt = 1;
        }
        long p = v.entry[t];
        for (;;) {
            const long q = il2p_next_tag(s_m, len, p);
            if (q >= len) break;
            if (lane == cnt) { mine = i0 + q; have = true; }
            ++cnt;
            p = q + IL2P_STATES;
        }
        const bool want = have && mine + IL2P_HEADER_BITS < v.n;       // its 120th bit lies in this push
        Il2pRec r{};
        if (want) r = il2p_record(v.bits, IL2P_CARRY + mine, (u64)((long long)v.pos0 + mine), (unsigned)c);
        const u64 wm = __ballot(want);
        if (wm && lane == __ffsll(wm) - 1) atomicAdd(a.stats + 2 * c, (u64)__popcll(wm));
        wave_append(want, r, a.count, a.recs, (u64)a.rec_cap);
        __syncthreads();
    }
}

// x workgroups per stream for `per_stream` tiles each: all of them while the device has room, else a share of eight per CU
static unsigned il2p_grid_x(long per_stream, long nstreams) {
    const long room = ((long)device_cu_count() * 8 + nstreams - 1) / nstreams;
    return (unsigned)std::max<long>(1, std::min(per_stream, room));
}

void launch_il2p(const Il2pArgs& a, hipStream_t s) {
    if (a.n_cap <= 0 || a.nstreams <= 0) return;
    const unsigned ns = (unsigned)a.nstreams, gx = il2p_grid_x(a.ntiles, a.nstreams);
    hipLaunchKernelGGL(k_il2p_mark, dim3(gx, ns), dim3(IL2P_B), 0, s, a);
    hipLaunchKernelGGL(k_il2p_scan, dim3(1, ns), dim3(IL2P_SB), 0, s, a);
    hipLaunchKernelGGL(k_il2p_emit, dim3(gx, ns), dim3(64), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
