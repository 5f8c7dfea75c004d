// kernels_pwm.hip — the end of examples/restaurant_pager.rs:
//   [ComplexToMag2 (src/complex_to_mag2.rs:8-21)] -> PwmDecoder (src/pwm_decoder.rs:385-513)
// over the next n samples of a stream (the arithmetic is pwm_core.hpp's).  A sample is one of four maps on
// {low, high}; the maps of a tile of PWM_T samples compose, so the slicer is a scan:
//   k_pwm_classify   the samples, read ONCE: their classes packed (2 bits each) and the tile's map
//   k_pwm_scan       ONE workgroup: the state in front of every tile, from the carried one
//   k_pwm_mark       the tile's states from the packed classes: its edges as bits, and their count
//   k_pwm_offs       ONE workgroup: the edges in front of every tile
//   k_pwm_edges      the edges in stream order
//   k_pwm_table      the carried candidate table copied to the half this push writes
//   k_pwm_walk       ONE wave: 64 items (falls) at a time are made by its lanes, then taken in order — the bit into the open frame,
//                    the frame against the candidate table (the lanes compare hashes, then bits), the deliveries at a reset —
//                    and what the next push starts from
// No workgroup waits on another; the grids depend on n and the settings alone.  Seven launches whatever the samples hold.
#include "kernels.hpp"
#include "packet_common.hpp"
#include "pwm_core.hpp"

namespace rr {

static_assert(sizeof(PwmRec) == 24, "PwmRec is rr_pwm_frame");

struct PwmSrcF32 {
    const float* p;
    __device__ __forceinline__ float load(long i) const { return p[i]; }
};
// norm_sqr with the reference's three f32 roundings (kernels_burst.hip's loader)
struct PwmSrcMag2 {
    const cf* p;
    __device__ __forceinline__ float load(long i) const {
        const cf z = p[i];
        return add_rn(mul_rn(z.x, z.x), mul_rn(z.y, z.y));
    }
};

struct PwmCompose { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return pwm_compose(a, b); } };
struct PwmAdd { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a + b; } };

// Inclusive scan over a workgroup of NW waves, `op(left, right)` associative with identity `ident`; s_w: NW words.
// -> this thread's inclusive value; total: the whole workgroup's.
template <int NW, class Op> __device__ __forceinline__ unsigned pwm_block_scan(unsigned v, unsigned ident, unsigned* s_w, Op op, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned u = __shfl_up(v, off, 64);
        if (lane >= off) v = op(u, v);
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    unsigned pre = ident, tot = ident;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const unsigned t = s_w[k];
        if (k < w) pre = op(pre, t);
        tot = op(tot, t);
    }
    __syncthreads();                          // s_w is free again
    total = tot;
    return op(pre, v);
}
template <class Op> __device__ __forceinline__ unsigned pwm_exclusive(unsigned incl, unsigned ident, unsigned* s_x, Op) {
    // the inclusive value of the thread in front (a workgroup-wide shift through LDS)
    s_x[threadIdx.x] = incl;
    __syncthreads();
    const unsigned e = threadIdx.x ? s_x[threadIdx.x - 1] : ident;
    __syncthreads();
    return e;
}

template <class SRC> __global__ __launch_bounds__(PWM_B) void k_pwm_classify(SRC src, PwmArgs a) {
    __shared__ unsigned char s_c[PWM_T];
    __shared__ unsigned s_w[PWM_B / 64];
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long o0 = tile * PWM_T;
#pragma unroll
        for (int i = 0; i < PWM_PER; ++i) {
            const int j = i * PWM_B + threadIdx.x;
            // (behind the push's last sample: the identity, which moves no state and makes no edge)
            s_c[j] = o0 + j < a.n ? (unsigned char)pwm_class(src.load(o0 + j), a.cfg.high_thr, a.cfg.low_thr) : (unsigned char)PWM_ID;
        }
        __syncthreads();
        unsigned c16 = 0;
#pragma unroll
        for (int i = 0; i < PWM_PER; ++i) c16 |= (unsigned)s_c[threadIdx.x * PWM_PER + i] << (2 * i);
        a.cls[tile * PWM_B + threadIdx.x] = (unsigned short)c16;
        unsigned total;
        pwm_block_scan<PWM_B / 64>(pwm_compose8(c16), PWM_ID, s_w, PwmCompose{}, total);
        if (threadIdx.x == 0) a.tmap[tile] = (unsigned char)total;
        // (pwm_block_scan's last barrier stands between these reads of s_c and the next tile's writes)
    }
}

// tstate[t] = the state in front of tile t
__global__ __launch_bounds__(PWM_SB) void k_pwm_scan(PwmArgs a) {
    __shared__ unsigned s_w[PWM_SB / 64];
    __shared__ unsigned s_x[PWM_SB];
    unsigned state = a.st_in->high ? 1u : 0u;
    for (long c0 = 0; c0 < a.ntiles; c0 += PWM_SB) {
        const long t = c0 + threadIdx.x;
        unsigned total;
        const unsigned incl = pwm_block_scan<PWM_SB / 64>(t < a.ntiles ? a.tmap[t] : PWM_ID, PWM_ID, s_w, PwmCompose{}, total);
        const unsigned excl = pwm_exclusive(incl, PWM_ID, s_x, PwmCompose{});
        if (t < a.ntiles) a.tstate[t] = (unsigned char)pwm_apply(excl, state);
        state = pwm_apply(total, state);
    }
}

__global__ __launch_bounds__(PWM_B) void k_pwm_mark(PwmArgs a) {
    __shared__ unsigned s_w[PWM_B / 64];
    __shared__ unsigned s_x[PWM_B];
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const unsigned c16 = a.cls[tile * PWM_B + threadIdx.x];
        unsigned total;
        const unsigned incl = pwm_block_scan<PWM_B / 64>(pwm_compose8(c16), PWM_ID, s_w, PwmCompose{}, total);
        const unsigned excl = pwm_exclusive(incl, PWM_ID, s_x, PwmCompose{});
        const unsigned s0 = pwm_apply(excl, a.tstate[tile]);
        const unsigned e8 = pwm_edges8(pwm_states8(c16, s0), s0);
        a.ebits[tile * PWM_B + threadIdx.x] = (unsigned char)e8;
        unsigned cnt;
        pwm_block_scan<PWM_B / 64>((unsigned)__popc(e8), 0u, s_w, PwmAdd{}, cnt);
        if (threadIdx.x == 0) a.tilecnt[tile] = cnt;
    }
}

// offs[t] = the edges in front of tile t; *etotal = all of them
__global__ __launch_bounds__(PWM_SB) void k_pwm_offs(PwmArgs a) {
    __shared__ unsigned s_w[PWM_SB / 64];
    unsigned base = 0;
    for (long c0 = 0; c0 < a.ntiles; c0 += PWM_SB) {
        const long t = c0 + threadIdx.x;
        const unsigned v = t < a.ntiles ? a.tilecnt[t] : 0u;
        unsigned total;
        const unsigned incl = pwm_block_scan<PWM_SB / 64>(v, 0u, s_w, PwmAdd{}, total);
        if (t < a.ntiles) a.offs[t] = base + incl - v;
        base += total;
    }
    if (threadIdx.x == 0) a.etotal[0] = base;
}

__global__ __launch_bounds__(PWM_B) void k_pwm_edges(PwmArgs a) {
    __shared__ unsigned s_w[PWM_B / 64];
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        unsigned e8 = a.ebits[tile * PWM_B + threadIdx.x];
        const unsigned cnt = (unsigned)__popc(e8);
        unsigned total;
        const unsigned incl = pwm_block_scan<PWM_B / 64>(cnt, 0u, s_w, PwmAdd{}, total);
        unsigned long long at = (unsigned long long)a.offs[tile] + incl - cnt;
        const unsigned long long p0 = (unsigned long long)tile * PWM_T + threadIdx.x * PWM_PER;
        while (e8) {
            const int i = __ffs((int)e8) - 1;
            e8 &= e8 - 1;
            if (at < (unsigned long long)a.ecap && p0 + i < (unsigned long long)a.n) a.edges[at] = (unsigned)(p0 + i);
            ++at;
        }
    }
}

// rows [0, ncand) of the carried candidate table -> the half this push writes
__global__ __launch_bounds__(PWM_B) void k_pwm_table(PwmArgs a) {
    const unsigned nc = min(a.st_in->ncand, a.cfg.max_distinct);
    const unsigned long long words = (unsigned long long)nc * (a.pitch / 8);
    const unsigned long long* in = reinterpret_cast<const unsigned long long*>(a.cand_in);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(a.cand_out);
    for (unsigned long long i = (unsigned long long)blockIdx.x * PWM_B + threadIdx.x; i < words; i += (unsigned long long)gridDim.x * PWM_B)
        out[i] = in[i];
}

constexpr int PWM_MAXB = 16384, PWM_MAXD = 1024;      // pwm_host.hpp refuses beyond them

// what the one wave of k_pwm_walk holds for pwm_step.  Everything is wave-uniform; the lanes split the comparisons and the copies.
struct PwmWaveOps {
    const PwmArgs& a;
    unsigned char* s_bits;
    PwmCand* s_cand;
    unsigned ncand;
    unsigned long long nout, abits;
    int lane;
    __device__ __forceinline__ void put_bit(unsigned idx, unsigned bit) {
        if (lane == 0) s_bits[idx] = (unsigned char)bit;
    }
    // a byte of the table this push writes, as the other lanes left it
    __device__ __forceinline__ unsigned row_byte(unsigned row, unsigned i) const {
        return __hip_atomic_load(a.cand_out + (unsigned long long)row * a.pitch + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ void candidate(unsigned len, unsigned long long first, unsigned long long hash) {
        __syncthreads();                      // (one wave: lane 0's bits are in LDS)
        int found = -1;
        for (unsigned base = 0; base < ncand && found < 0; base += 64) {
            const unsigned i = base + lane;
            bool m = i < ncand && s_cand[i].len == len && s_cand[i].hash == hash;
            if (m)
                for (unsigned k = 0; k < len; ++k)
                    if (row_byte(i, k) != s_bits[k]) { m = false; break; }
            const unsigned long long mask = __ballot(m);
            if (mask) found = (int)base + __ffsll((long long)mask) - 1;
        }
        if (found >= 0) {
            if (lane == 0 && s_cand[found].repeats != 0xffffffffu) s_cand[found].repeats++;
        } else if (ncand < a.cfg.max_distinct) {
            for (unsigned k = lane; k < len; k += 64) a.cand_out[(unsigned long long)ncand * a.pitch + k] = s_bits[k];
            if (lane == 0) { s_cand[ncand].first = first; s_cand[ncand].hash = hash; s_cand[ncand].len = len; s_cand[ncand].repeats = 1; }
            ncand++;
            __threadfence();
        }
        __syncthreads();
    }
    __device__ void deliver() {
        __syncthreads();
        for (unsigned i = 0; i < ncand; ++i) {
            const PwmCand c = s_cand[i];
            if (c.repeats < a.cfg.min_repeats) continue;
            if (nout < (unsigned long long)a.rec_cap && abits + c.len <= (unsigned long long)a.arena_cap) {
                for (unsigned k = lane; k < c.len; k += 64) a.arena[abits + k] = (unsigned char)row_byte(i, k);
                if (lane == 0) {
                    PwmRec r;
                    r.first_sample = c.first; r.start = abits; r.len = c.len; r.repeats = c.repeats;
                    a.recs[nout] = r;
                }
            }
            nout++;
            abits += c.len;
        }
        ncand = 0;
        __syncthreads();
    }
};

__device__ __forceinline__ unsigned long long pwm_readlane64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return (unsigned long long)hi << 32 | lo;
}

__global__ __launch_bounds__(64) void k_pwm_walk(PwmArgs a) {
    __shared__ unsigned char s_bits[PWM_MAXB];
    __shared__ PwmCand s_cand[PWM_MAXD];
    const int lane = threadIdx.x;
    const PwmState st = *a.st_in;
    const unsigned long long n = (unsigned long long)a.n;
    const unsigned long long ne = a.eof ? 0ull : min(a.etotal[0], (unsigned long long)a.ecap);
    const unsigned nc0 = min(st.ncand, a.cfg.max_distinct), fc0 = min(st.fcount, a.cfg.max_bits);
    for (unsigned i = lane; i < nc0; i += 64) s_cand[i] = a.meta_in[i];
    for (unsigned i = lane; i < fc0; i += 64) s_bits[i] = a.fbits_in[i];
    __syncthreads();
    PwmWaveOps ops{a, s_bits, s_cand, nc0, 0ull, 0ull, lane};
    PwmWalk w;
    pwm_walk_load(w, st);
    w.fcount = fc0;
    const unsigned long long nitems = pwm_items(st, ne);
    for (unsigned long long base = 0; base < nitems; base += 64) {
        PwmItem mine;
        mine.flags = 0; mine.rise = 0; mine.width = 0;
        if (base + lane < nitems) mine = pwm_item(a.cfg, st, a.edges, ne, n, base + lane);
        const int cnt = (int)min(64ull, nitems - base);
        for (int l = 0; l < cnt; ++l) {
            PwmItem it;
            // (lane l's item as wave-uniform scalars: the branches of pwm_step are scalar, and no lane waits for a shuffle)
            it.flags = (unsigned)__builtin_amdgcn_readlane((int)mine.flags, l);
            it.rise = pwm_readlane64(mine.rise, l);
            it.width = pwm_readlane64(mine.width, l);
            pwm_step(a.cfg, w, it, ops);
        }
    }
    pwm_walk_tail(w, st, a.edges, ne);
    if (a.eof) ops.deliver();                 // finalize_eof (:612-618): the candidates go, the open frame is thrown away
    __syncthreads();
    for (unsigned i = lane; i < ops.ncand; i += 64) a.meta_out[i] = s_cand[i];
    for (unsigned i = lane; i < w.fcount; i += 64) a.fbits_out[i] = s_bits[i];
    if (lane == 0) {
        PwmState o;
        pwm_state_out(o, st, w, a.edges, ne, n, ops.ncand, a.eof || st.eof ? 1u : 0u);
        *a.st_out = o;
        a.count[0] = ops.nout;
        a.count[1] = ops.abits;
    }
}

void launch_pwm(const PwmArgs& a, hipStream_t s) {
    if (a.eof) {
        hipLaunchKernelGGL(k_pwm_table, dim3(tiles_grid(((long)a.cfg.max_distinct * (long)(a.pitch / 8) + PWM_B - 1) / PWM_B)), dim3(PWM_B), 0, s, a);
        hipLaunchKernelGGL(k_pwm_walk, dim3(1), dim3(64), 0, s, a);
        RR_HIP(hipGetLastError());
        return;
    }
    if (a.n <= 0) return;
    const unsigned gt = tiles_grid(a.ntiles);
    if (a.es == 8) hipLaunchKernelGGL((k_pwm_classify<PwmSrcMag2>), dim3(gt), dim3(PWM_B), 0, s, PwmSrcMag2{static_cast<const cf*>(a.in)}, a);
    else hipLaunchKernelGGL((k_pwm_classify<PwmSrcF32>), dim3(gt), dim3(PWM_B), 0, s, PwmSrcF32{static_cast<const float*>(a.in)}, a);
    hipLaunchKernelGGL(k_pwm_scan, dim3(1), dim3(PWM_SB), 0, s, a);
    hipLaunchKernelGGL(k_pwm_mark, dim3(gt), dim3(PWM_B), 0, s, a);
    hipLaunchKernelGGL(k_pwm_offs, dim3(1), dim3(PWM_SB), 0, s, a);
    hipLaunchKernelGGL(k_pwm_edges, dim3(gt), dim3(PWM_B), 0, s, a);
    hipLaunchKernelGGL(k_pwm_table, dim3(tiles_grid(((long)a.cfg.max_distinct * (long)(a.pitch / 8) + PWM_B - 1) / PWM_B)), dim3(PWM_B), 0, s, a);
    hipLaunchKernelGGL(k_pwm_walk, dim3(1), dim3(64), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
