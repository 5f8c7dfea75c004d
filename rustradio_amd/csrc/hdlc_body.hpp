// hdlc_body.hpp — the bodies of the seven HdlcDeframer kernels as __device__ functions, shared by
//   kernels_hdlc.hip     one stream, its bits one byte each (rr_hdlc_deframer)
//   kernels_hdlcrx.hip   N streams of f32 symbols with the bit chain in front (rr_hdlc_receiver)
// A body works on ONE stream: an HdlcArgs is the view of it (the one-stream kernels get theirs from the host, the N-stream ones
// build stream blockIdx.y's from base pointers and pitches).  Two things differ between the users and are template parameters:
//   Src   how the mark stage gets the tile's 64 words of virtual bits and the 8 bits in front of them into LDS:
//           src.fill(a, C, nv, t0, s_raw, s_prev), called by all HD_B threads; it ends with a __syncthreads()
//   Sink  where a delivered frame's record goes: sink.record(a, pos, start, len, flags), called by one lane; `start` is relative
//         to a.arena
// Every body strides over its work with blockIdx.x / gridDim.x alone, so the y dimension is the caller's.
#pragma once
#include "hdlc_core.hpp"
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
constexpr int HD_B = 256;                     // threads of a tile's workgroup
constexpr int HD_W = HDLC_T / 64;             // words of a tile
constexpr int HD_SB = 1024;                   // threads of the two scan kernels
static_assert(HDLC_T == 16 * HD_B && HD_W == 64, "hd_mark_body: 16 bits per thread, one word per lane of a wave");
static_assert(HDLC_GB == HD_B, "hd_gap_body: one gap per thread");

__device__ __forceinline__ long hd_carried(const HdlcArgs& a) {
    const long c = (long)a.st_in->count;
    return c < a.carry_cap ? c : a.carry_cap;
}
__device__ __forceinline__ long hd_nv(const HdlcArgs& a) {
    const long nv = hd_carried(a) + a.n;
    return nv < a.nv_max ? nv : a.nv_max;
}
__device__ __forceinline__ long hd_ends(const HdlcArgs& a) {
    const u64 e = *a.etotal;
    return e < (u64)a.ends_cap ? (long)e : a.ends_cap;
}
// the bits of word w that lie inside the gap (s, f)
__device__ __forceinline__ u64 hd_gap_mask(long w, long s, long f) {
    const long lo = s + 1 > (w << 6) ? s + 1 : (w << 6), hi = f < ((w + 1) << 6) ? f : ((w + 1) << 6);
    if (lo >= hi) return 0ull;
    const long k = hi - (w << 6);
    return (~0ull << (lo & 63)) & (k == 64 ? ~0ull : (1ull << k) - 1ull);
}
__device__ __forceinline__ hdlc_map hd_wave_scan_maps(hdlc_map v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const hdlc_map u = __shfl_up(v, o, 64);
        if (lane >= o) v = hdlc_map_then(u, v);
    }
    return v;
}

// The byte source: bit v of the virtual stream is cin[v] in front of the push's own bits[v - C]; one ballot per 64 bits.
struct HdlcByteSrc {
    static __device__ __forceinline__ bool bit(const HdlcArgs& a, long C, long nv, long v) {
        if (v < 0 || v >= nv) return false;
        return ((v < C ? a.cin[v] : a.bits[v - C]) & 1u) != 0;
    }
    __device__ __forceinline__ void fill(const HdlcArgs& a, long C, long nv, long t0, u64* s_raw, u64* s_prev) const {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const u64 b = __ballot(bit(a, C, nv, t0 + i * HD_B + tid));
            if (lane == 0) s_raw[i * (HD_B / 64) + wave] = b;
        }
        if (wave == 0) {                       // the 8 bits in front of the tile
            const u64 h = __ballot(lane < 8 && bit(a, C, nv, t0 - 8 + lane));
            if (lane == 0) *s_prev = h << 56;
        }
        __syncthreads();
    }
};
// The one-stream record: rr_hdlc_frame, appended to a.recs.
struct HdlcRecSink {
    __device__ __forceinline__ void record(const HdlcArgs& a, u64 pos, u64 start, unsigned len, unsigned flags) const {
        const u64 slot = atomicAdd(a.count, 1ull);
        if (slot < (u64)a.rec_cap) a.recs[slot] = HdlcRec{pos, start, len, flags};
    }
};

// reset_count / reset_stats: this workgroup is the one that zeroes *a.count / a.pstats[0 .. 3) for the push (the kernels that
// add to them are launched later).
template <class Src>
__device__ __forceinline__ void hd_mark_body(const HdlcArgs& a, const Src& src, bool reset_count, bool reset_stats) {
    __shared__ u64 s_raw[HD_W];
    __shared__ u64 s_prev;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long C = hd_carried(a), nv = hd_nv(a);
    if (tid == 0) {
        if (reset_count) *a.count = 0;
        if (reset_stats) a.pstats[0] = a.pstats[1] = a.pstats[2] = 0;
    }
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long t0 = tile * HDLC_T;
        src.fill(a, C, nv, t0, s_raw, &s_prev);
        if (wave == 0) {
            const u64 cur = s_raw[lane], prev = lane ? s_raw[lane - 1] : s_prev;
            HdlcMarks m = hdlc_marks(cur, prev);
            const long v0 = t0 + 64 * lane;    // features exist at HDLC_HALO <= v < nv: the halo's own are the previous push's
            u64 valid = v0 >= nv ? 0ull : (nv - v0 >= 64 ? ~0ull : (1ull << (nv - v0)) - 1ull);
            if (v0 == 0) valid &= ~0ull << HDLC_HALO;
            m.flag &= valid; m.abort &= valid; m.stuffed &= valid;
            const long w = tile * HD_W + lane;
            a.raw[w] = cur; a.fl[w] = m.flag; a.ab[w] = m.abort; a.sf[w] = m.stuffed;
            unsigned cnt = (unsigned)hdlc_popc(m.flag);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0) a.tilecnt[tile] = cnt;
        }
        __syncthreads();                      // the next tile overwrites the shared arrays
    }
}

__device__ __forceinline__ void hd_offs_body(const HdlcArgs& a) {
    __shared__ u64 s_w[HD_SB / 64];
    __shared__ u64 s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (long c0 = 0; c0 < a.ntiles; c0 += HD_SB) {
        const long t = c0 + tid;
        const u64 mine = t < a.ntiles ? a.tilecnt[t] : 0ull;
        u64 inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        u64 before = s_run;
        for (int q = 0; q < wave; ++q) before += s_w[q];
        if (t < a.ntiles) a.offs[t] = before + inc - mine;
        __syncthreads();                      // everyone has read s_run and s_w
        if (tid == HD_SB - 1) s_run = before + inc;
        __syncthreads();
    }
    if (tid == 0) *a.etotal = s_run;
}

__device__ __forceinline__ void hd_ends_body(const HdlcArgs& a) {
    const int lane = threadIdx.x;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long w = tile * HD_W + lane;
        u64 f = a.fl[w];
        const u64 mine = (u64)hdlc_popc(f);
        u64 inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        u64 at = a.offs[tile] + inc - mine;
        for (; f; f &= f - 1, ++at)
            if (at < (u64)a.ends_cap) a.ends[at] = (unsigned)((w << 6) + hdlc_ctz(f));     // (always: flag ends are 7 bits apart)
    }
}

__device__ __forceinline__ void hd_gap_body(const HdlcArgs& a) {
    __shared__ hdlc_map s_w[HDLC_GB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long E = hd_ends(a), nb = (E + HDLC_GB - 1) / HDLC_GB;
    for (long b = blockIdx.x; b < nb; b += gridDim.x) {
        const long j = b * HDLC_GB + tid;
        hdlc_map m = HDLC_MAP_ID;
        if (j < E) {
            const long s = j ? (long)a.ends[j - 1] : HDLC_HALO - 1, f = (long)a.ends[j];
            m = hdlc_gap_scan(a.ab, a.sf, s, f, a.max_size).map;
            a.gmap[j] = (unsigned char)m;
        }
        const hdlc_map inc = hd_wave_scan_maps(m & HDLC_MAP_MASK, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        hdlc_map before = HDLC_MAP_ID;
        for (int q = 0; q < wave; ++q) before = hdlc_map_then(before, s_w[q]);
        hdlc_map prev = __shfl_up(inc, 1, 64);
        if (lane == 0) prev = HDLC_MAP_ID;
        if (j < E) a.pmap[j] = (unsigned char)hdlc_map_then(before, prev);         // the gaps of the block in front of this one
        if (tid == HDLC_GB - 1) a.bmap[b] = (unsigned char)hdlc_map_then(before, inc);
        __syncthreads();                      // the next block overwrites s_w
    }
}

__device__ __forceinline__ void hd_resolve_body(const HdlcArgs& a) {
    __shared__ hdlc_map s_w[HD_SB / 64];
    __shared__ hdlc_map s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long E = hd_ends(a), nb = (E + HDLC_GB - 1) / HDLC_GB;
    const int st0 = a.st_in->state == HDLC_S ? HDLC_S : a.st_in->state == HDLC_U3 ? HDLC_U3 : HDLC_U;
    if (tid == 0) s_run = HDLC_MAP_ID;
    __syncthreads();
    for (long c0 = 0; c0 < nb; c0 += HD_SB) {
        const long i = c0 + tid;
        const hdlc_map mine = i < nb ? (hdlc_map)a.bmap[i] & HDLC_MAP_MASK : HDLC_MAP_ID;
        const hdlc_map inc = hd_wave_scan_maps(mine, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        hdlc_map before = s_run;
        for (int q = 0; q < wave; ++q) before = hdlc_map_then(before, s_w[q]);
        hdlc_map prev = __shfl_up(inc, 1, 64);
        if (lane == 0) prev = HDLC_MAP_ID;
        if (i < nb) a.bstate[i] = (unsigned char)hdlc_map_at(hdlc_map_then(before, prev), st0);
        __syncthreads();                      // everyone has read s_run and s_w
        if (tid == HD_SB - 1) s_run = hdlc_map_then(before, inc);
        __syncthreads();
    }
    if (tid == 0) *a.fin = hdlc_map_at(s_run, st0);
}

template <class Sink>
__device__ __forceinline__ void hd_emit_body(const HdlcArgs& a, const Sink& sink) {
    const int lane = threadIdx.x & 63;
    const long E = hd_ends(a), C = hd_carried(a);
    const long nwaves = (long)gridDim.x * (HD_B / 64);
    for (long j = (long)blockIdx.x * (HD_B / 64) + (threadIdx.x >> 6); j < E; j += nwaves) {      // (uniform over the wave)
        if (!(a.gmap[j] & HDLC_EMITS)) continue;
        if (hdlc_map_at(a.pmap[j], a.bstate[j / HDLC_GB]) != HDLC_S) continue;
        const long s = j ? (long)a.ends[j - 1] : HDLC_HALO - 1, f = (long)a.ends[j];
        // the gap's words in 64 segments, one per lane: the kept bits of each and in front of each
        const long wf = (s + 1) >> 6, wl = (f - 1) >> 6, seg = (wl - wf + 64) / 64;
        u64 mine_kept = 0;
        for (long w = wf + lane * seg; w < wf + (lane + 1) * seg && w <= wl; ++w) mine_kept += (u64)hdlc_popc(~a.sf[w] & hd_gap_mask(w, s, f));
        u64 upto = mine_kept;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 u = __shfl_up(upto, o, 64);
            if (lane >= o) upto += u;
        }
        const u64 before = upto - mine_kept, kept = __shfl(upto, 63, 64);
        const long nbytes = hdlc_frame_bytes(kept, a.min_size);
        if (nbytes < 0 || (!a.keep && nbytes < 2)) continue;
        const u64 pos = a.w0 + (u64)f - (u64)C, start = (u64)(s + 1) / 8;
        const long blen = a.keep ? nbytes : nbytes - 2;              // the bytes delivered
        const long ch = (nbytes + 63) / 64;
        const long k0 = lane * ch < nbytes ? lane * ch : nbytes, k1 = k0 + ch < nbytes ? k0 + ch : nbytes;
        unsigned fcs = 0xffffu, got = 0;
        // the segment that holds the lane's first kept bit (every lane takes the six steps: they read one another's `before`)
        const int sj = hdlc_seg_find(8 * (u64)k0, [&](int j) { return __shfl(before, j, 64); });
        const u64 sb = __shfl(before, sj, 64);
        if (k0 < k1) {
            const long p = hdlc_select(a.sf, hdlc_seg_from(s, wf, seg, sj), f, 8 * (u64)k0 - sb);
            HdlcCursor c = hdlc_cursor(a.raw, a.sf, p < 0 ? s + 1 : p);
            for (long k = k0; k < k1 && p >= 0; ++k) {
                const unsigned byte = hdlc_take_byte(a.raw, a.sf, c);
                if (k < blen) {
                    if ((long)start + k < a.arena_cap) a.arena[start + k] = (unsigned char)byte;       // (always: hdlc_host.hpp's bound)
                    fcs = crc16_byte(fcs, byte);
                } else {
                    got |= byte << (8 * (unsigned)(k - blen));       // low byte first
                }
            }
        }
        if (a.keep) {
            if (lane == 0) { sink.record(a, pos, start, (unsigned)blen, 0u); atomicAdd(a.pstats + 0, 1ull); }
            continue;
        }
        const long c0 = k0 < blen ? k0 : blen, c1 = k1 < blen ? k1 : blen;            // the lane's bytes under the CRC
        unsigned diff = (c0 < c1 ? hdlc_crc_part(fcs, (u64)(blen - c1)) : 0u) ^ got;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) diff ^= __shfl_xor(diff, o, 64);
        if (diff == 0) {
            if (lane == 0) { sink.record(a, pos, start, (unsigned)blen, 0u); atomicAdd(a.pstats + 0, 1ull); }
            continue;
        }
        if (!a.fix) {
            if (lane == 0) atomicAdd(a.pstats + 1, 1ull);
            continue;
        }
        const long mine = hdlc_syn_search(diff, 8 * (u64)blen, 8 * (u64)c0, 8 * (u64)c1);
        long hit = mine < 0 ? 0x7fffffffffffffffl : mine;            // the lowest byte and bit, as find_right_crc's loop leaves it
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long other = __shfl_xor(hit, o, 64);
            hit = other < hit ? other : hit;
        }
        if (hit != 0x7fffffffffffffffl) {
            if (mine == hit && (long)start + hit / 8 < a.arena_cap) a.arena[start + hit / 8] ^= (unsigned char)(1u << (hit & 7));   // (the lane stored that byte itself)
            if (lane == 0) { sink.record(a, pos, start, (unsigned)blen, 1u); atomicAdd(a.pstats + 0, 1ull); atomicAdd(a.pstats + 2, 1ull); }
        } else if (lane == 0) {
            if (hdlc_popc(diff) == 1) atomicAdd(a.pstats + 2, 1ull);                 // one wrong bit in the CRC field: counted twice, nothing delivered
            atomicAdd(a.pstats + 1, 1ull);
        }
    }
}

__device__ __forceinline__ void hd_carry_body(const HdlcArgs& a) {
    const int tid = threadIdx.x;
    const long E = hd_ends(a), nv = hd_nv(a);
    const long last = E ? (long)a.ends[E - 1] : HDLC_HALO - 1;
    const HdlcCarry c = hdlc_carry_plan(last, *a.fin, nv, a.max_size);
    const long cnt = c.count < a.carry_cap ? c.count : a.carry_cap;       // (always: hdlc_carry_bits is the bound)
    for (long i = tid; i < cnt; i += HD_B) {
        const long v = c.from + i;
        a.cout[i] = (unsigned char)(a.raw[v >> 6] >> (v & 63) & 1ull);
    }
    if (tid == 0) {
        HdlcState st;
        for (int k = 0; k < 3; ++k) st.stats[k] = a.st_in->stats[k] + a.pstats[k];
        st.count = (unsigned)cnt;
        st.state = c.state;
        *a.st_out = st;
    }
}

}  // namespace rr
