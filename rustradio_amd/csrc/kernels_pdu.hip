// kernels_pdu.hip — the middle of the burst receivers (examples/ax25-9600-wpcr.rs:103-139): the comparison of BurstTagger
// (src/burst_tagger.rs:68-85), StreamToPdu (src/stream_to_pdu.rs:198-275) and Midpointer (src/wpcr.rs:62-78) over one window of a
// data / trigger stream pair, and PduToStream (src/pdu_to_stream.rs:57-101) over a batch of Wpcr's symbols.
//
// StreamToPdu fed alternating edges has a closed form.  With the rising edges r_j, their falling edges f_j,
// L = f_j - r_j and free = 0 at the start of the stream: a rising edge below `free` is ignored with its falling edge; an accepted
// one with L + tail <= max_size files [r_j, f_j + tail) and sets free = f_j + tail; any other accepted one files nothing and sets
// free = r_j + max_size + 1.  So every rising edge j has ONE successor whatever happened before it — nxt(j), the first rising edge
// at or behind the `free` that accepting j leaves — and the accepted edges of a window are the chain j0, nxt(j0), nxt(nxt(j0)) ..
// from the first edge j0 at or behind the carried `free`.  nxt is monotone (nxt(j) > j), so:
//   k_pdu_tiles<false>  per tile the number of threshold crossings; the window is copied behind the open burst into the arena
//   k_pdu_count         ... the same for Complex data (StreamToPdu<Complex>), or with no copy (the burst saver, kernels_saver.hip)
//   (offsets)           the crossings in front of every tile: launch_bits_tag_offsets, one workgroup
//   k_pdu_tiles<true>   every tile writes its crossings, ascending, at its offset: the edge list, (pos << 1) | cur
//   k_pdu_next          nxt(j) by binary search in the edge list, one thread per rising edge; the carried burst meets the window's
//                       first edge; mark = {j0}
//   k_pdu_jump          ceil(log2 R) rounds of pointer doubling.  Round k: every marked j marks jmp[j], then jmp[j] = jmp[jmp[j]]
//                       (into the other buffer).  Before round k the chain's members at distance < 2^k from j0 are marked, after it
//                       those at distance < 2^(k+1).  Work O(R log R), depth O(log R) launches.
//   k_pdu_emit          every marked edge whose PDU is complete appends one record; the chain's last member leaves the state
//   k_pdu_midpoint      one workgroup per record: the mean (f64 tree sum), then a radix select of two ranks, 8 bits per pass
// No thread walks the edge list, no workgroup waits on another: the order is the stream's.  The host enqueues the same launches
// whatever the trigger holds (it does not know the edge count): a launch whose round is beyond the window's chain returns at once.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
constexpr int PDU_B = 256;                    // threads of a workgroup
constexpr int PDU_PER = PDU_T / PDU_B;        // consecutive trigger samples of one thread
static_assert(PDU_PER == 8 && PDU_B % 64 == 0, "k_pdu_tiles: 8 samples per thread");
constexpr int PDU_MB = 1024;                  // k_pdu_midpoint: threads of the workgroup that owns a burst

__device__ __forceinline__ long pdu_min(long a, long b) { return a < b ? a : b; }

template <bool WRITE> __global__ __launch_bounds__(PDU_B) void k_pdu_tiles(PduArgs a) {
    __shared__ unsigned s_w[PDU_B / 64];
    const long ntiles = (a.n + PDU_T - 1) / PDU_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool last_in = a.st_in->last != 0;
    if (!WRITE) {
        // the open burst: its samples so far end the previous arena; they go in front of arena[C)
        const u64 orr = a.st_in->open_r;
        long clen = (orr == PDU_NONE || !a.prev_arena) ? 0 : (long)(a.w0 - orr);
        clen = pdu_min(clen, a.C);
        for (long k = (long)blockIdx.x * PDU_B + tid; k < clen; k += (long)gridDim.x * PDU_B) {
            const long idx = a.C - clen + k;
            static_cast<float*>(a.arena)[idx] = static_cast<const float*>(a.prev_arena)[idx + a.n_prev];
        }
    }
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long o0 = tile * PDU_T;
        const int cnt = (int)pdu_min(a.n - o0, PDU_T);
        if (!WRITE)
            for (int j = tid; j < cnt; j += PDU_B) static_cast<float*>(a.arena)[a.C + o0 + j] = static_cast<const float*>(a.data)[o0 + j];
        const long i0 = o0 + (long)tid * PDU_PER;
        bool prev = i0 == 0 ? last_in : (i0 - 1 < a.n ? a.trig[i0 - 1] > a.thr : false);
        unsigned em = 0, cm = 0;
#pragma unroll
        for (int i = 0; i < PDU_PER; ++i) {
            if (i0 + i < a.n) {
                const bool cur = a.trig[i0 + i] > a.thr;          // (NaN: not above)
                if (cur != prev) em |= 1u << i;
                if (cur) cm |= 1u << i;
                prev = cur;
                if (!WRITE && i0 + i == a.n - 1) a.st_out->last = cur ? 1 : 0;
            }
        }
        const unsigned mine = (unsigned)__popc(em);
        unsigned inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < PDU_B / 64; ++q) {
            if (q < w) before += s_w[q];
            total += s_w[q];
        }
        if (!WRITE) {
            if (tid == 0) a.tilecnt[tile] = total;
        } else {
            u64 slot = a.offs[tile] + before + inc - mine;
#pragma unroll
            for (int i = 0; i < PDU_PER; ++i)
                if (em >> i & 1u) {
                    if (slot < (u64)a.n) a.edges[slot] = ((unsigned)(i0 + i) << 1) | (cm >> i & 1u);
                    ++slot;
                }
        }
        __syncthreads();                      // the next tile overwrites s_w
    }
}

// k_pdu_tiles<false> for the handles whose data is not f32: the same tile counts and the same `last`, with the two copies made
// in Complex samples (COPY: a StreamToPdu<Complex> handle) or not at all (the burst saver has filled the arena itself).  A kernel
// of its own so that the f32 handle's code object stays what it was.
template <bool COPY> __global__ __launch_bounds__(PDU_B) void k_pdu_count(PduArgs a) {
    __shared__ unsigned s_w[PDU_B / 64];
    const long ntiles = (a.n + PDU_T - 1) / PDU_T;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool last_in = a.st_in->last != 0;
    cf* const arena = static_cast<cf*>(a.arena);
    if (COPY) {
        const cf* const prev = static_cast<const cf*>(a.prev_arena);
        const u64 orr = a.st_in->open_r;
        long clen = (orr == PDU_NONE || !prev) ? 0 : (long)(a.w0 - orr);
        clen = pdu_min(clen, a.C);
        for (long k = (long)blockIdx.x * PDU_B + tid; k < clen; k += (long)gridDim.x * PDU_B) {
            const long idx = a.C - clen + k;
            arena[idx] = prev[idx + a.n_prev];
        }
    }
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long o0 = tile * PDU_T;
        const int cnt = (int)pdu_min(a.n - o0, PDU_T);
        if (COPY)
            for (int j = tid; j < cnt; j += PDU_B) arena[a.C + o0 + j] = static_cast<const cf*>(a.data)[o0 + j];
        const long i0 = o0 + (long)tid * PDU_PER;
        bool prev = i0 == 0 ? last_in : (i0 - 1 < a.n ? a.trig[i0 - 1] > a.thr : false);
        unsigned mine = 0;
#pragma unroll
        for (int i = 0; i < PDU_PER; ++i) {
            if (i0 + i < a.n) {
                const bool cur = a.trig[i0 + i] > a.thr;              // (NaN: not above)
                if (cur != prev) ++mine;
                prev = cur;
                if (i0 + i == a.n - 1) a.st_out->last = cur ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if (lane == 0) s_w[w] = mine;
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
#pragma unroll
            for (int q = 0; q < PDU_B / 64; ++q) total += s_w[q];
            a.tilecnt[tile] = total;
        }
        __syncthreads();                      // the next tile overwrites s_w
    }
}

// the window's edge list as rising / falling pairs: rising edge j is entry base + 2 j, its falling edge the next entry
struct PduEdges {
    const unsigned* e;
    long E, base, R;
    __device__ __forceinline__ long rpos(long j) const { return (long)(e[base + 2 * j] >> 1); }
    // the first k in [lo, R) with rpos(k) >= key
    __device__ __forceinline__ long lower_bound(long lo, long key) const {
        long hi = R;
        while (lo < hi) {
            const long mid = lo + (hi - lo) / 2;
            if (rpos(mid) < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
};
__device__ __forceinline__ PduEdges pdu_edges(const PduArgs& a) {
    PduEdges g;
    g.e = a.edges;
    const u64 et = *a.etotal;
    g.E = et < (u64)a.n ? (long)et : a.n;
    g.base = a.st_in->last ? 1 : 0;           // inside a burst: the first edge falls, and belongs to no rising edge of the window
    g.R = (g.E - g.base + 1) / 2;
    return g;
}
// the successor's key of rising edge j (relative to the window, clamped to n) and what the edge is
struct PduEdge {
    long rp, fp, key;
    bool hasf, sized;
};
__device__ __forceinline__ PduEdge pdu_edge(const PduArgs& a, const PduEdges& g, long j) {
    PduEdge d;
    d.rp = g.rpos(j);
    const long fi = g.base + 2 * j + 1;
    d.hasf = fi < g.E;
    d.fp = d.hasf ? (long)(g.e[fi] >> 1) : a.n;
    d.sized = d.hasf && (u64)(d.fp - d.rp) + a.tail <= a.max_size;
    const u64 k = d.sized ? (u64)d.fp + a.tail : (u64)d.rp + a.max_size + 1;
    d.key = d.hasf ? (long)(k < (u64)a.n ? k : (u64)a.n) : a.n;
    return d;
}

__global__ __launch_bounds__(PDU_B) void k_pdu_next(PduArgs a) {
    __shared__ PduRoot s_root;
    const PduEdges g = pdu_edges(a);
    if (threadIdx.x == 0) {
        PduRoot r;
        r.free = a.st_in->free;
        r.open_r = a.st_in->open_r;
        r.open_f = a.st_in->open_f;
        if (r.open_r != PDU_NONE && r.open_f == PDU_NONE && g.E > 0) {        // the open burst's falling edge: the window's first
            const u64 f = a.w0 + (g.e[0] >> 1);
            if (f - r.open_r + a.tail <= a.max_size) { r.open_f = f; r.free = f + a.tail; }
            else { r.free = r.open_r + a.max_size + 1; r.open_r = PDU_NONE; }
        }
        const u64 rel = r.free > a.w0 ? r.free - a.w0 : 0;
        r.R = g.R;
        r.j0 = g.lower_bound(0, (long)(rel < (u64)a.n ? rel : (u64)a.n));
        s_root = r;
        if (blockIdx.x == 0) *a.root = r;
    }
    __syncthreads();
    const long j0 = s_root.j0;
    for (long j = (long)blockIdx.x * PDU_B + threadIdx.x; j < g.R; j += (long)gridDim.x * PDU_B) {
        const PduEdge d = pdu_edge(a, g, j);
        a.jmp0[j] = (unsigned)(d.hasf ? g.lower_bound(j + 1, d.key) : g.R);
        a.mark[j] = j == j0 ? 1u : 0u;
    }
}

__global__ __launch_bounds__(PDU_B) void k_pdu_jump(const PduRoot* __restrict__ root, const unsigned* __restrict__ jin,
                                                    unsigned* __restrict__ jout, unsigned* mark, int k) {
    const long R = root->R;
    if ((1L << k) >= R) return;               // no member of the chain is that far from j0
    for (long j = (long)blockIdx.x * PDU_B + threadIdx.x; j < R; j += (long)gridDim.x * PDU_B) {
        const unsigned t = jin[j];
        if (t < R) {
            if (mark[j]) mark[t] = 1u;
            jout[j] = jin[t];
        } else {
            jout[j] = (unsigned)R;
        }
    }
}

__device__ __forceinline__ PduRec pdu_rec(const PduArgs& a, u64 r_abs, u64 len) {
    PduRec rec;
    rec.start = (u64)((long)(r_abs - a.w0) + a.C);                // (a burst begun earlier: a negative offset from the window)
    rec.len = len;
    rec.stream_pos = r_abs;
    rec.ok = 1;
    rec.mean = rec.mid = 0.0f;
    rec.nlow = 0;
    return rec;
}

__global__ __launch_bounds__(PDU_B) void k_pdu_emit(PduArgs a) {
    const PduEdges g = pdu_edges(a);
    const PduRoot rt = *a.root;
    const u64 wend = a.w0 + (u64)a.n;
    const long total_len = a.C + a.n;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bool filed = false;
        if (rt.open_r != PDU_NONE && rt.open_f != PDU_NONE && rt.open_f + a.tail <= wend) {      // the carried burst is whole
            const PduRec rec = pdu_rec(a, rt.open_r, rt.open_f + a.tail - rt.open_r);
            if ((long)rec.start >= 0 && (long)(rec.start + rec.len) <= total_len) {
                const u64 slot = atomicAdd(a.count, 1ull);
                if (slot < (u64)a.rec_cap) a.recs[slot] = rec;
            }
            filed = true;
        }
        if (rt.j0 >= g.R) {                   // no rising edge of the window is accepted: the state is the carried one's
            u64 fr = rt.free, orr = PDU_NONE, of = PDU_NONE;
            if (rt.open_r != PDU_NONE) {
                if (rt.open_f != PDU_NONE) { if (!filed) { orr = rt.open_r; of = rt.open_f; } }
                else if (wend - rt.open_r > a.max_size) fr = rt.open_r + a.max_size + 1;          // too long whatever follows
                else orr = rt.open_r;
            }
            a.st_out->free = fr; a.st_out->open_r = orr; a.st_out->open_f = of;
        }
    }
    for (long b0 = (long)blockIdx.x * PDU_B; b0 < g.R; b0 += (long)gridDim.x * PDU_B) {
        const long j = b0 + threadIdx.x;
        bool e = false;
        PduRec rec{};
        if (j < g.R && a.mark[j]) {
            const PduEdge d = pdu_edge(a, g, j);
            const u64 r_abs = a.w0 + (u64)d.rp;
            const bool complete = d.sized && (u64)d.fp + a.tail <= (u64)a.n;
            if (complete) {
                rec = pdu_rec(a, r_abs, (u64)(d.fp - d.rp) + a.tail);
                e = (long)(rec.start + rec.len) <= total_len;
            }
            if (!d.hasf || j == g.R - 1 || g.rpos(g.R - 1) < d.key) {          // the chain ends here
                u64 fr, orr = PDU_NONE, of = PDU_NONE;
                if (!d.hasf) {
                    if ((u64)(a.n - d.rp) > a.max_size) fr = r_abs + a.max_size + 1;
                    else { fr = rt.free; orr = r_abs; }
                } else if (d.sized && !complete) {
                    fr = a.w0 + (u64)d.fp + a.tail; orr = r_abs; of = a.w0 + (u64)d.fp;
                } else {
                    fr = d.sized ? a.w0 + (u64)d.fp + a.tail : r_abs + a.max_size + 1;
                }
                a.st_out->free = fr; a.st_out->open_r = orr; a.st_out->open_f = of;
            }
        }
        wave_append(e, rec, a.count, a.recs, (u64)a.rec_cap);
    }
}

// ---- Midpointer (wpcr.rs:62-78) -------------------------------------------------------------------------------------------------------
// the order of f32::total_cmp as an unsigned integer
__device__ __forceinline__ unsigned pdu_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pdu_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// One histogram increment per active lane; every lane of the wave calls it.  An NRZ burst puts a whole wave on one or two bins
// (two levels): the first two distinct digits of the wave are counted by one lane each, only what is left adds per lane.
__device__ __forceinline__ void pdu_hist_add(unsigned* h, bool act, unsigned d) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const u64 m = __ballot(act);
        if (m == 0) return;
        const int leader = __ffsll(m) - 1;
        const unsigned dl = __shfl(d, leader, 64);
        const u64 same = __ballot(act && d == dl);
        if (lane == leader) atomicAdd(&h[dl], (unsigned)__popcll(same));
        if (d == dl) act = false;
    }
    if (act) atomicAdd(&h[d], 1u);
}
// Threads [0, 256) serve rank 0 on hist[0], threads [256, 512) rank 1 on hist[h1]: the bin that holds the rank extends the prefix.
__device__ __forceinline__ void pdu_select(unsigned (*hist)[256], int h1, unsigned* s_pref, u64* s_rank) {
    const int tid = threadIdx.x, r = tid >> 8, d = tid & 255;
    bool hit = false;
    unsigned pf = 0;
    u64 rest = 0;
    if (tid < 512) {
        const unsigned* h = hist[r ? h1 : 0];
        const u64 rk = s_rank[r];
        pf = s_pref[r];
        u64 pre = 0;
        for (int q = 0; q < d; ++q) pre += h[q];
        hit = rk >= pre && rk < pre + h[d];
        rest = rk - pre;
    }
    __syncthreads();                          // everyone has read the rank it divides
    if (hit) { s_pref[r] = (pf << 8) | (unsigned)d; s_rank[r] = rest; }
    __syncthreads();
}

__global__ __launch_bounds__(PDU_MB) void k_pdu_midpoint(const float* __restrict__ arena, PduRec* recs, const u64* __restrict__ count,
                                                         long rec_cap, float* __restrict__ ranks) {
    __shared__ unsigned s_hist[2][256];
    __shared__ double s_red[PDU_MB / 64];
    __shared__ u64 s_cnt[PDU_MB / 64];
    __shared__ unsigned s_pref[2];
    __shared__ u64 s_rank[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 cn = *count;
    const long nrec = cn < (u64)rec_cap ? (long)cn : rec_cap;
    for (long rec = blockIdx.x; rec < nrec; rec += gridDim.x) {
        const float* x = arena + recs[rec].start;
        const long len = (long)recs[rec].len;
        // the mean: an f64 tree sum in an order that depends on len alone
        double s = 0.0;
        for (long i = tid; i < len; i += PDU_MB) s += (double)x[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) s_red[w] = s;
        if (tid < 512) s_hist[tid >> 8][tid & 255] = 0;
        __syncthreads();
        double S = 0.0;
        for (int q = 0; q < PDU_MB / 64; ++q) S += s_red[q];
        const float mean = (float)(S / (double)len);
        // nlow and the histogram of the keys' top byte
        u64 c = 0;
        if (mean == mean)
            for (long i0 = 0; i0 < len; i0 += PDU_MB) {
                const long i = i0 + tid;
                const bool act = i < len;
                const float v = act ? x[i] : 0.0f;
                if (act && !(v > mean)) ++c;
                pdu_hist_add(s_hist[0], act, pdu_key(v) >> 24);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[w] = c;
        __syncthreads();
        u64 nlow = 0;
        for (int q = 0; q < PDU_MB / 64; ++q) nlow += s_cnt[q];
        if (!(mean == mean) || nlow == 0 || nlow == (u64)len) {                // Midpointer pushes nothing
            if (tid == 0) {
                recs[rec].ok = 0; recs[rec].mean = mean; recs[rec].mid = 0.0f; recs[rec].nlow = mean == mean ? nlow : (u64)len;
                ranks[2 * rec] = ranks[2 * rec + 1] = 0.0f;
            }
            __syncthreads();                  // the next record overwrites the shared arrays
            continue;
        }
        if (tid == 0) { s_pref[0] = s_pref[1] = 0; s_rank[0] = nlow / 2; s_rank[1] = nlow + ((u64)len - nlow) / 2; }
        __syncthreads();
        pdu_select(s_hist, 0, s_pref, s_rank);
        for (int shift = 16; shift >= 0; shift -= 8) {
            if (tid < 512) s_hist[tid >> 8][tid & 255] = 0;
            __syncthreads();
            const unsigned p0 = s_pref[0], p1 = s_pref[1];
            for (long i0 = 0; i0 < len; i0 += PDU_MB) {
                const long i = i0 + tid;
                const bool act = i < len;
                const unsigned key = pdu_key(act ? x[i] : 0.0f), hi = key >> (shift + 8), d = key >> shift & 255u;
                pdu_hist_add(s_hist[0], act && hi == p0, d);
                pdu_hist_add(s_hist[1], act && hi == p1, d);
            }
            __syncthreads();
            pdu_select(s_hist, 1, s_pref, s_rank);
        }
        if (tid == 0) {
            const float low = pdu_unkey(s_pref[0]), high = pdu_unkey(s_pref[1]);
            recs[rec].ok = 1;
            recs[rec].mean = mean;
            recs[rec].mid = add_rn(low, mul_rn(sub_rn(high, low), 0.5f));       // low + (high - low) / 2.0, three f32 roundings
            recs[rec].nlow = nlow;
            ranks[2 * rec] = low;             // (rr_debug_pdu_ranks)
            ranks[2 * rec + 1] = high;
        }
        __syncthreads();
    }
}

void launch_pdu(const PduArgs& a, hipStream_t s, int elem) {
    if (a.n <= 0) return;
    if (elem != PDU_F32 && a.midpoint) throw Error("Midpointer is a block over f32");
    const long ntiles = (a.n + PDU_T - 1) / PDU_T;
    const unsigned gt = tiles_grid(ntiles);
    RR_HIP(hipMemsetAsync(a.count, 0, sizeof(u64), s));
    if (elem == PDU_F32) hipLaunchKernelGGL((k_pdu_tiles<false>), dim3(gt), dim3(PDU_B), 0, s, a);
    else if (elem == PDU_C32) hipLaunchKernelGGL((k_pdu_count<true>), dim3(gt), dim3(PDU_B), 0, s, a);
    else hipLaunchKernelGGL((k_pdu_count<false>), dim3(gt), dim3(PDU_B), 0, s, a);
    launch_bits_tag_offsets(a.tilecnt, ntiles, a.offs, a.etotal, s);
    hipLaunchKernelGGL((k_pdu_tiles<true>), dim3(gt), dim3(PDU_B), 0, s, a);
    const long maxr = a.n / 2 + 1;            // rising edges a window of n samples can hold
    const unsigned gr = tiles_grid((maxr + PDU_B - 1) / PDU_B);
    hipLaunchKernelGGL(k_pdu_next, dim3(gr), dim3(PDU_B), 0, s, a);
    int k = 0;
    for (; (1L << k) < maxr; ++k)
        hipLaunchKernelGGL(k_pdu_jump, dim3(gr), dim3(PDU_B), 0, s, (const PduRoot*)a.root, (const unsigned*)(k & 1 ? a.jmp1 : a.jmp0),
                           k & 1 ? a.jmp0 : a.jmp1, a.mark, k);
    hipLaunchKernelGGL(k_pdu_emit, dim3(gr), dim3(PDU_B), 0, s, a);
    if (a.midpoint) {
        const unsigned gm = (unsigned)std::max<long>(1, std::min(a.rec_cap, (long)std::max(1, device_cu_count()) * 2));
        hipLaunchKernelGGL(k_pdu_midpoint, dim3(gm), dim3(PDU_MB), 0, s, (const float*)a.arena, a.recs, (const u64*)a.count, a.rec_cap,
                           a.ranks);
    }
    RR_HIP(hipGetLastError());
}

// ---- PduToStream over a batch (pdu_to_stream.rs:57-101) --------------------------------------------------------------------------------
__global__ __launch_bounds__(PDU_B) void k_pdu_pack(const float* __restrict__ syms, const long* __restrict__ desc, long nb, long total,
                                                    float* __restrict__ out) {
    for (long o = (long)blockIdx.x * PDU_B + threadIdx.x; o < total; o += (long)gridDim.x * PDU_B) {
        long lo = 0, hi = nb;                 // the last burst whose dst is <= o
        while (hi - lo > 1) {
            const long mid = lo + (hi - lo) / 2;
            if (desc[3 * mid + 1] <= o) lo = mid; else hi = mid;
        }
        out[o] = syms[desc[3 * lo] + (o - desc[3 * lo + 1])];
    }
}
void launch_pdu_pack(const float* syms, const long* desc, long nb, long total, float* out, hipStream_t s) {
    if (total <= 0 || nb <= 0) return;
    const unsigned grid = tiles_grid((total + PDU_B - 1) / PDU_B);
    hipLaunchKernelGGL(k_pdu_pack, dim3(grid), dim3(PDU_B), 0, s, syms, desc, nb, total, out);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
