// kernels_kiss.hip — the KISS blocks of the two modem examples (examples/bell202.rs, examples/g3ruh.rs; the
// arithmetic is kiss_core.hpp's).
//
// Decode: KissFrame (src/kiss.rs:165-228) -> KissDecode (:96-137) over the carried bytes followed by the window, in tiles of
// KISS_T bytes, 16 per thread.  A gap is closed by its FEND, and everything that FEND has to know is a difference of sums that
// run over the whole stream (FESC bytes, bad escapes) plus where the FEND in front of it stands — one associative KissSum:
//   k_kiss_sum           every tile's KissSum
//   k_kiss_scan          ONE workgroup scans them: the summary in front of every tile, and of the whole push
//   k_kiss_pass<1>       every FEND judges its gap (kiss_close); the tile's packets, bytes and counters
//   k_kiss_scan2         ONE workgroup: the packets and bytes in front of every tile, the totals, the next state
//   k_kiss_pass<2>       every delivering FEND writes its record; one that closes a gap from an earlier tile says where it goes
//   k_kiss_pass<3>       every kept byte stores itself at its gap's base + its rank; the open gap's bytes go to the next carry
// Encode: KissEncode (:247-286) -> PduToStream over the packets' bytes back to back, in tiles of KISS_T:
//   k_kenc_count         the escaped bytes of every tile
//   k_kenc_scan          ONE workgroup: those in front of every tile
//   k_kenc_emit          every byte stores itself (and its FESC) at 3 p + 2 + g + C(g); the tile's packet boundaries store the FENDs
//                        and the port byte around them
// No workgroup waits on another, nothing is added to an output atomically, and every output byte has one writer.
#include "kiss_core.hpp"
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
constexpr int KS_B = 256;                     // threads of a workgroup
constexpr int KS_W = KS_B / 64;
constexpr int KS_SB = 1024;                   // threads of the scan kernels
constexpr unsigned KS_NOBASE = 0xffffffffu;
static_assert(KISS_T == KS_B * KISS_LANE && KISS_LANE == 16, "16 bytes per thread");
static_assert(sizeof(KissSum) == 6 * sizeof(unsigned), "KissArgs::sums: six words per tile");

struct KsPair { unsigned a, b; };
struct KsFive { unsigned v[5]; };
struct KsAddPair { __device__ KsPair operator()(const KsPair& x, const KsPair& y) const { return KsPair{x.a + y.a, x.b + y.b}; } };
struct KsAddFive {
    __device__ KsFive operator()(const KsFive& x, const KsFive& y) const {
        KsFive r;
#pragma unroll
        for (int q = 0; q < 5; ++q) r.v[q] = x.v[q] + y.v[q];
        return r;
    }
};
struct KsCombine { __device__ KissSum operator()(const KissSum& x, const KissSum& y) const { return kiss_combine(x, y); } };

template <class T> __device__ __forceinline__ T ks_shfl_up(const T& v, int o) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    union { T t; unsigned w[sizeof(T) / 4]; } in, out;
    in.t = v;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) out.w[i] = __shfl_up(in.w[i], o, 64);
    return out.t;
}
// inclusive scan over the wave, in lane order
template <class T, class Op> __device__ __forceinline__ T ks_wave_scan(T v, int lane, Op op) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = ks_shfl_up(v, o);
        if (lane >= o) v = op(u, v);
    }
    return v;
}
// Exclusive scan over the workgroup's NW waves, in thread order; *total: the workgroup's.  Every thread calls it; s_w is free again
// on return.
template <int NW, class T, class Op> __device__ __forceinline__ T ks_block_scan(const T& mine, const T& identity, T* s_w, Op op, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = ks_wave_scan(mine, lane, op);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    T before = identity, all = identity;
    for (int q = 0; q < NW; ++q) {
        if (q < wave) before = op(before, s_w[q]);
        all = op(all, s_w[q]);
    }
    T prev = ks_shfl_up(inc, 1);
    if (lane == 0) prev = identity;
    *total = all;
    __syncthreads();
    return op(before, prev);
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------------
struct KissV {                                // the virtual stream of a push
    const unsigned char* cin;
    const unsigned char* win;
    int c, len;
    __device__ __forceinline__ unsigned at(int v) const { return v < c ? cin[v] : win[v - c]; }
};
__device__ __forceinline__ int ks_code(const KissState* st) {
    const int code = st->code;
    return code == KISS_VIRT || code == KISS_OVER ? code : KISS_UNSYNC;
}
__device__ __forceinline__ KissV ks_virtual(const KissArgs& a) {
    long c = ks_code(a.st_in) == KISS_VIRT ? (long)a.st_in->carry : 0;
    if (c > (long)a.max_len) c = a.max_len;
    if (c > a.nv_max - a.n) c = a.nv_max - a.n;                               // (the host's bound holds: never taken)
    return KissV{a.cin, a.bytes, (int)c, (int)(c + a.n)};
}
// the thread's bytes [v0, v0 + cnt), four to a word, the byte in front of them and the one behind
struct KissLane {
    unsigned w[4];
    unsigned prev, next;
    int v0, cnt;
    __device__ __forceinline__ unsigned byte(int k) const { return w[k >> 2] >> (8 * (k & 3)) & 0xffu; }
};
__device__ __forceinline__ KissLane ks_load(const KissV& V, long tile) {
    KissLane L;
    L.v0 = (int)(tile * KISS_T) + (int)threadIdx.x * KISS_LANE;
    const int left = V.len - L.v0;
    L.cnt = left < 0 ? 0 : left > KISS_LANE ? KISS_LANE : left;
    L.w[0] = L.w[1] = L.w[2] = L.w[3] = 0u;
    const unsigned char* p = V.win + (L.v0 - V.c);
    if (L.cnt == KISS_LANE && L.v0 >= V.c && (reinterpret_cast<size_t>(p) & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        L.w[0] = q.x; L.w[1] = q.y; L.w[2] = q.z; L.w[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < KISS_LANE; ++k)
            if (k < L.cnt) L.w[k >> 2] |= V.at(L.v0 + k) << (8 * (k & 3));
    }
    L.prev = L.cnt > 0 && L.v0 > 0 ? V.at(L.v0 - 1) : 0u;
    L.next = L.v0 + KISS_LANE < V.len ? V.at(L.v0 + KISS_LANE) : 0u;
    return L;
}
__device__ __forceinline__ KissSum ks_at(const KissV& V, const KissLane& L, int k) {
    const unsigned nx = k + 1 < KISS_LANE ? L.byte(k + 1 < KISS_LANE ? k + 1 : 0) : L.next;
    return kiss_byte(L.v0 + k, L.byte(k), nx, L.v0 + k + 1 < V.len);
}
__device__ __forceinline__ KissSum ks_lane_sum(const KissV& V, const KissLane& L) {
    KissSum s = kiss_none();
#pragma unroll
    for (int k = 0; k < KISS_LANE; ++k)
        if (k < L.cnt) s = kiss_combine(s, ks_at(V, L, k));
    return s;
}
// f(run, e, gap) at every FEND of the thread, run = the summary in front of it
template <class F> __device__ __forceinline__ void ks_fends(const KissV& V, const KissLane& L, KissSum run, unsigned max_len, F&& f) {
#pragma unroll
    for (int k = 0; k < KISS_LANE; ++k) {
        if (k < L.cnt) {
            if (L.byte(k) == KISS_FEND) {
                const long glen = kiss_gap_len(run, L.v0 + k);
                const unsigned port = glen >= 1 && glen <= (long)max_len ? V.at(run.last + 1) : 0u;
                f(run, L.v0 + k, kiss_close(run, glen, max_len, port));
            }
            run = kiss_combine(run, ks_at(V, L, k));
        }
    }
}
__device__ __forceinline__ long ks_slot(int last) { return last < 0 ? 0 : (long)(last / KISS_T) + 1; }

__global__ __launch_bounds__(KS_B) void k_kiss_sum(KissArgs a) {
    __shared__ KissSum s_w[KS_W];
    const KissV V = ks_virtual(a);
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const KissLane L = ks_load(V, tile);
        KissSum all;
        ks_block_scan<KS_W>(ks_lane_sum(V, L), kiss_none(), s_w, KsCombine(), &all);
        if (threadIdx.x == 0) reinterpret_cast<KissSum*>(a.sums)[tile] = all;
    }
}

__global__ __launch_bounds__(KS_SB) void k_kiss_scan(KissArgs a) {
    __shared__ KissSum s_w[KS_SB / 64];
    __shared__ KissSum s_run;
    const int tid = threadIdx.x;
    const KissSum* sums = reinterpret_cast<const KissSum*>(a.sums);
    if (tid == 0) s_run = kiss_seed(ks_code(a.st_in));
    __syncthreads();
    for (long c0 = 0; c0 < a.ntiles; c0 += KS_SB) {
        const long t = c0 + tid;
        KissSum all;
        const KissSum ex = ks_block_scan<KS_SB / 64>(t < a.ntiles ? sums[t] : kiss_none(), kiss_none(), s_w, KsCombine(), &all);
        const KissSum run = s_run;
        if (t < a.ntiles) reinterpret_cast<KissSum*>(a.tin)[t] = kiss_combine(run, ex);
        __syncthreads();                      // everyone has read s_run
        if (tid == 0) s_run = kiss_combine(run, all);
        __syncthreads();
    }
    if (tid == 0) *reinterpret_cast<KissSum*>(a.root) = s_run;
}

template <int PH> __global__ __launch_bounds__(KS_B) void k_kiss_pass(KissArgs a) {
    __shared__ KissSum s_w[KS_W];
    __shared__ KsFive s_w5[KS_W];
    __shared__ KsPair s_w2[KS_W];
    __shared__ unsigned s_base[PH == 3 ? KISS_T : 1];     // where the gap closed by the tile's k-th FEND goes
    const int tid = threadIdx.x;
    const KissV V = ks_virtual(a);
    const unsigned max_len = a.max_len;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const KissLane L = ks_load(V, tile);
        const KissSum tin = reinterpret_cast<const KissSum*>(a.tin)[tile];
        KissSum all;
        const KissSum ex = kiss_combine(tin, ks_block_scan<KS_W>(ks_lane_sum(V, L), kiss_none(), s_w, KsCombine(), &all));
        KsFive cnt{{0u, 0u, 0u, 0u, 0u}};
        ks_fends(V, L, ex, max_len, [&](const KissSum&, int, const KissGap& g) {
            if (g.kind == KISS_G_DELIVERED) { cnt.v[0] += 1u; cnt.v[1] += g.len; }
            else if (g.kind != KISS_G_NOTHING) cnt.v[g.kind] += 1u;
        });
        if (PH == 1) {
            KsFive tot;
            ks_block_scan<KS_W>(cnt, KsFive{{0u, 0u, 0u, 0u, 0u}}, s_w5, KsAddFive(), &tot);
            if (tid < 5) a.tsum[5 * tile + tid] = tot.v[tid];
            continue;
        }
        KsPair tot2;
        const KsPair at = ks_block_scan<KS_W>(KsPair{cnt.v[0], cnt.v[1]}, KsPair{0u, 0u}, s_w2, KsAddPair(), &tot2);
        unsigned pk = a.toff[2 * tile] + at.a, by = a.toff[2 * tile + 1] + at.b;
        ks_fends(V, L, ex, max_len, [&](const KissSum& run, int e, const KissGap& g) {
            const bool keep = g.kind == KISS_G_DELIVERED;
            if (PH == 2 && keep) {
                if ((long)pk < a.rec_cap) a.recs[pk] = KissRec{a.w0 + (u64)(e - V.c), (u64)by, g.len, g.in_bytes, g.port, 0u};
                const long slot = ks_slot(run.last);
                if (slot != tile + 1) a.obase[slot] = by;                     // (slot <= tile: the opening FEND stands in front of e)
            }
            if (PH == 3) s_base[run.nfend - tin.nfend] = keep ? by : KS_NOBASE;
            if (keep) { pk += 1u; by += g.len; }
        });
        if (PH == 3) {
            __syncthreads();
            KissSum run = ex;
#pragma unroll
            for (int k = 0; k < KISS_LANE; ++k) {
                if (k < L.cnt) {
                    const unsigned cur = L.byte(k);
                    unsigned rank, value;
                    if (cur != KISS_FEND && run.last >= KISS_VIRT && kiss_emit(run, L.v0 + k, k ? L.byte(k ? k - 1 : 0) : L.prev, cur, &rank, &value)) {
                        const unsigned kf = run.nfend - tin.nfend;            // its closing FEND: the tile's kf-th, or a later tile's
                        const unsigned base = kf < all.nfend ? s_base[kf] : a.obase[ks_slot(run.last)];
                        if (base != KS_NOBASE && (long)base + (long)rank < a.arena_cap) a.arena[base + rank] = (unsigned char)value;
                    }
                    run = kiss_combine(run, ks_at(V, L, k));
                }
            }
            __syncthreads();                  // the next tile overwrites s_base
        }
    }
    if (PH == 3) {                            // the next carry: read from this push's virtual stream, written to the other half
        int code;
        unsigned carry;
        kiss_next(*reinterpret_cast<const KissSum*>(a.root), V.len, max_len, &code, &carry);
        for (long i = (long)blockIdx.x * KS_B + tid; i < (long)carry; i += (long)gridDim.x * KS_B) a.cout[i] = (unsigned char)V.at(V.len - (int)carry + (int)i);
    }
}

__global__ __launch_bounds__(KS_SB) void k_kiss_scan2(KissArgs a) {
    __shared__ KsFive s_w[KS_SB / 64];
    __shared__ KsFive s_run;
    const int tid = threadIdx.x;
    if (tid == 0) s_run = KsFive{{0u, 0u, 0u, 0u, 0u}};
    __syncthreads();
    for (long c0 = 0; c0 < a.ntiles; c0 += KS_SB) {
        const long t = c0 + tid;
        KsFive mine{{0u, 0u, 0u, 0u, 0u}}, all;
        if (t < a.ntiles)
            for (int q = 0; q < 5; ++q) mine.v[q] = a.tsum[5 * t + q];
        const KsFive ex = ks_block_scan<KS_SB / 64>(mine, KsFive{{0u, 0u, 0u, 0u, 0u}}, s_w, KsAddFive(), &all);
        const KsFive run = s_run;
        if (t < a.ntiles) { a.toff[2 * t] = run.v[0] + ex.v[0]; a.toff[2 * t + 1] = run.v[1] + ex.v[1]; }
        __syncthreads();                      // everyone has read s_run
        if (tid == 0) s_run = KsAddFive()(run, all);
        __syncthreads();
    }
    if (tid == 0) {
        const KissV V = ks_virtual(a);
        const KsFive t = s_run;
        KissState st = *a.st_in;
        st.stats[0] += (u64)t.v[0] + t.v[2] + t.v[3];
        st.stats[1] += t.v[0];
        st.stats[2] += t.v[2];
        st.stats[3] += t.v[3];
        st.stats[4] += t.v[4];
        kiss_next(*reinterpret_cast<const KissSum*>(a.root), V.len, a.max_len, &st.code, &st.carry);
        *a.st_out = st;
        a.count[0] = t.v[0];
        a.count[1] = t.v[1];
    }
}

void launch_kiss_decode(const KissArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    const unsigned gt = tiles_grid(a.ntiles);
    hipLaunchKernelGGL(k_kiss_sum, dim3(gt), dim3(KS_B), 0, s, a);
    hipLaunchKernelGGL(k_kiss_scan, dim3(1), dim3(KS_SB), 0, s, a);
    hipLaunchKernelGGL(k_kiss_pass<1>, dim3(gt), dim3(KS_B), 0, s, a);
    hipLaunchKernelGGL(k_kiss_scan2, dim3(1), dim3(KS_SB), 0, s, a);
    hipLaunchKernelGGL(k_kiss_pass<2>, dim3(gt), dim3(KS_B), 0, s, a);
    hipLaunchKernelGGL(k_kiss_pass<3>, dim3(gt), dim3(KS_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

// ---- encode ----------------------------------------------------------------------------------------------------------------------------
// the first b in [lo, hi) with pb[b] >= key (hi: none)
__device__ __forceinline__ long ke_lower(const u64* __restrict__ pb, long lo, long hi, u64 key) {
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (pb[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the first b in [lo, hi) with pb[b] > key
__device__ __forceinline__ long ke_upper(const u64* __restrict__ pb, long lo, long hi, u64 key) {
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (pb[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the thread's logical bytes [g0, g0 + cnt) of the batch and the packet of each: p[k] holds g0 + k (empty packets share their pb
// with the next one: the last of them holds the byte)
struct KencLane {
    unsigned char b[KISS_LANE];
    long g0, p0;
    int cnt;
};
__device__ __forceinline__ KencLane ke_load(const KissEncArgs& a, long tile) {
    KencLane L;
    L.g0 = tile * KISS_T + (long)threadIdx.x * KISS_LANE;
    const long left = a.nbytes - L.g0;
    L.cnt = left < 0 ? 0 : left > KISS_LANE ? KISS_LANE : (int)left;
    L.p0 = 0;
    if (L.cnt > 0) {
        long p = ke_upper(a.pb, 0, a.P + 1, (u64)L.g0) - 1;
        L.p0 = p;
        for (int k = 0; k < L.cnt; ++k) {
            const u64 g = (u64)(L.g0 + k);
            while (a.pb[p + 1] <= g) ++p;     // (pb[P] = nbytes > g)
            L.b[k] = a.bytes[a.starts[p] + (g - a.pb[p])];
        }
    }
    return L;
}
__device__ __forceinline__ unsigned ke_lane_count(const KencLane& L) {
    unsigned n = 0;
    for (int k = 0; k < L.cnt; ++k) n += kiss_escapes(L.b[k]);
    return n;
}
struct KsAdd { __device__ unsigned operator()(unsigned x, unsigned y) const { return x + y; } };

__global__ __launch_bounds__(KS_B) void k_kenc_count(KissEncArgs a) {
    __shared__ unsigned s_w[KS_W];
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const KencLane L = ke_load(a, tile);
        unsigned all;
        ks_block_scan<KS_W>(ke_lane_count(L), 0u, s_w, KsAdd(), &all);
        if (threadIdx.x == 0) a.tcnt[tile] = all;
    }
}
__global__ __launch_bounds__(KS_SB) void k_kenc_scan(KissEncArgs a) {
    __shared__ unsigned s_w[KS_SB / 64];
    __shared__ unsigned s_run;
    const int tid = threadIdx.x;
    if (tid == 0) s_run = 0u;
    __syncthreads();
    for (long c0 = 0; c0 < a.ntiles; c0 += KS_SB) {
        const long t = c0 + tid;
        unsigned all;
        const unsigned ex = ks_block_scan<KS_SB / 64>(t < a.ntiles ? a.tcnt[t] : 0u, 0u, s_w, KsAdd(), &all);
        const unsigned run = s_run;
        if (t < a.ntiles) a.tin[t] = run + ex;
        __syncthreads();                      // everyone has read s_run
        if (tid == 0) s_run = run + all;
        __syncthreads();
    }
}
__global__ __launch_bounds__(KS_B) void k_kenc_emit(KissEncArgs a) {
    __shared__ unsigned s_w[KS_W];
    __shared__ long s_b[2];
    __shared__ unsigned s_cnt[KISS_T + 1];    // C at every byte of the tile and behind its last
    const int tid = threadIdx.x;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long tb0 = tile * KISS_T;
        if (tid == 0) {                       // the boundaries of the tile; the last tile: those at nbytes too
            s_b[0] = ke_lower(a.pb, 0, a.P + 1, (u64)tb0);
            s_b[1] = tile == a.ntiles - 1 ? a.P + 1 : ke_lower(a.pb, 0, a.P + 1, (u64)(tb0 + KISS_T));
        }
        const KencLane L = ke_load(a, tile);
        unsigned all;
        unsigned C = a.tin[tile] + ks_block_scan<KS_W>(ke_lane_count(L), 0u, s_w, KsAdd(), &all);
        long p = L.p0;
        for (int k = 0; k < KISS_LANE; ++k) {
            s_cnt[tid * KISS_LANE + k] = C;
            if (k < L.cnt) {
                const u64 g = (u64)(L.g0 + k);
                while (a.pb[p + 1] <= g) ++p;
                const long pos = 3 * p + 2 + (long)g + (long)C;
                const unsigned b = L.b[k];
                if (kiss_escapes(b)) {
                    if (pos + 1 < a.cap) { a.out[pos] = (unsigned char)KISS_FESC; a.out[pos + 1] = (unsigned char)(b == KISS_FEND ? KISS_TFEND : KISS_TFESC); }
                    ++C;
                } else if (pos < a.cap) {
                    a.out[pos] = (unsigned char)b;
                }
            }
        }
        if (tid == KS_B - 1) s_cnt[KISS_T] = C;
        __syncthreads();
        const long b_lo = s_b[0], b_hi = s_b[1];
        for (long b = b_lo + tid; b < b_hi; b += KS_B) {
            const u64 gb = a.pb[b];
            const u64 o = gb - (u64)tb0;                                      // 0 .. KISS_T: a byte of this tile, or nbytes behind the last
            const unsigned Cb = s_cnt[o < (u64)KISS_T ? o : (u64)KISS_T];
            a.cb[b] = Cb;
            const long pos = 3 * b + (long)gb + (long)Cb;                     // packet b's opening FEND; packet b - 1's closing one in front
            if (b > 0 && pos - 1 < a.cap) a.out[pos - 1] = (unsigned char)KISS_FEND;
            if (b < a.P && pos + 1 < a.cap) { a.out[pos] = (unsigned char)KISS_FEND; a.out[pos + 1] = (unsigned char)kiss_port_byte(a.ports[b]); }
        }
        if (tile == a.ntiles - 1 && tid == 0) *a.total = (u64)(3 * a.P + a.nbytes) + s_cnt[KISS_T];
        __syncthreads();                      // the next tile overwrites the shared arrays
    }
}

void launch_kiss_encode(const KissEncArgs& a, hipStream_t s) {
    if (a.P <= 0) return;
    const unsigned gt = tiles_grid(a.ntiles);
    hipLaunchKernelGGL(k_kenc_count, dim3(gt), dim3(KS_B), 0, s, a);
    hipLaunchKernelGGL(k_kenc_scan, dim3(1), dim3(KS_SB), 0, s, a);
    hipLaunchKernelGGL(k_kenc_emit, dim3(gt), dim3(KS_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
