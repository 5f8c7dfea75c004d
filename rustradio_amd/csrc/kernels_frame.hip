// kernels_frame.hip — the front of the packet transmitters (examples/g3ruh.rs:250-267, examples/bell202.rs:160-176):
//   FcsAdder (src/hdlc_framer.rs:28-42) -> HdlcFramer (hdlc_encode, :60-86) -> PduToStream<u8> (src/pdu_to_stream.rs:57-101)
//   -> Scrambler::g3ruh (src/descrambler.rs:41-47, 95-123) -> NrziEncode (src/nrzi.rs:52-69) -> Map(bit ? hi : lo)
// over a batch of packets of one byte buffer (the arithmetic is frame_core.hpp's).
//
// The framer.  The payload bits of all packets (FCS bytes included) stand back to back and are cut into tiles of FRAME_T bits.
// With C(g) = the stuffed bits behind payload bits before g and p(g) = the packet of bit g, payload bit g goes to
// 320 p(g) + 160 + g + C(g), the 0 stuffed behind it one further; the boundary in front of packet b (b = P: behind the last)
// owns the 320 flag bits around it — the closing flags of packet b - 1 and the opening flags of packet b, which lie back to
// back at 320 b - 160 + 8 pb[b] + C(8 pb[b]).  C is a scan of hdlc_encode's counter:
//   k_frame_crc_chunks   one lane per FRAME_CH bytes of a packet: its CRC times x^(8 bytes behind it)
//   k_frame_crc_fold     one wave per packet XORs its chunks
//   k_frame_sum          gathers the tile's bytes (payload or FCS) into one array and reduces their StuffSums to the tile's
//   k_frame_scan         ONE workgroup scans the tiles' summaries: the counter and C in front of every tile
//   k_frame_emit         the same summaries scanned over the tile's threads; every thread walks its 16 bits and stores them,
//                        then the tile's boundaries store their flags and their C
// The line coder.  Tiles of LINE_T bits of the framed stream (or of a sync block's window):
//   k_line_z             every full tile's zero-state response -> the state it would leave behind, z
//   k_line_scan          ONE workgroup resolves c[t + 1] = M c[t] ^ z[t] with the powers of M
//   k_line_emit          the tile again with its true state in front; stores the bits or the levels
// No workgroup waits on another, nothing is added to the output atomically, and every output element has one writer.
#include "frame_core.hpp"
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

typedef unsigned long long u64;
constexpr int FR_B = 256;                     // threads of a workgroup
constexpr int FR_TB = FRAME_T / 8;            // bytes of a tile
constexpr int FR_SB = 1024;                   // threads of the two scan kernels
static_assert(FR_TB == 2 * FR_B, "k_frame_sum / k_frame_emit: two bytes per thread");
static_assert(LINE_T == 16 * FR_B && LINE_W == 64, "k_line_*: 16 bits per thread, one word per lane of a wave");

// the first b in [lo, hi) with pb[b] >= key (hi: none)
__device__ __forceinline__ long fr_lower(const u64* __restrict__ pb, long lo, long hi, u64 key) {
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (pb[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the first b in [lo, hi) with pb[b] > key
__device__ __forceinline__ long fr_upper(const u64* __restrict__ pb, long lo, long hi, u64 key) {
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (pb[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ StuffSum fr_shfl_up(const StuffSum& s, int o) {
    return StuffSum{__shfl_up(s.brk, o, 64), __shfl_up(s.lead, o, 64), __shfl_up(s.trail, o, 64), __shfl_up(s.stuffs, o, 64)};
}
// inclusive scan over the wave, in lane order
__device__ __forceinline__ StuffSum fr_wave_scan(StuffSum v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const StuffSum u = fr_shfl_up(v, o);
        if (lane >= o) v = stuff_combine(u, v);
    }
    return v;
}

// ---- CRC ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FR_B) void k_frame_crc_chunks(FrameArgs a) {
    for (long c = (long)blockIdx.x * FR_B + threadIdx.x; c < a.nchunks; c += (long)gridDim.x * FR_B) {
        const long p = fr_upper(a.cpre, 0, a.P + 1, (u64)c) - 1;          // (packets without chunks share their cpre with the next one)
        const u64 len = a.pb[p + 1] - a.pb[p] - 2;                         // (only launched with fcs)
        const u64 b0 = ((u64)c - a.cpre[p]) * FRAME_CH, b1 = b0 + FRAME_CH < len ? b0 + FRAME_CH : len;
        const unsigned char* x = a.bytes + a.starts[p];
        unsigned fcs = 0xffffu;
        for (u64 i = b0; i < b1; ++i) fcs = crc16_byte(fcs, x[i]);
        a.part[c] = crc16_mul(crc16_xpow8(len - b1), fcs ^ 0xffffu);
    }
}
__global__ __launch_bounds__(FR_B) void k_frame_crc_fold(FrameArgs a) {
    const int lane = threadIdx.x & 63;
    for (long p = (long)blockIdx.x * (FR_B / 64) + (threadIdx.x >> 6); p < a.P; p += (long)gridDim.x * (FR_B / 64)) {
        unsigned x = 0;
        for (u64 c = a.cpre[p] + lane; c < a.cpre[p + 1]; c += 64) x ^= a.part[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o, 64);
        if (lane == 0) a.crc[p] = x;           // (no chunks: 0, calc_crc of nothing)
    }
}

// ---- the stuffing scan ------------------------------------------------------------------------------------------------------------------
// logical byte G (< nbytes) of the batch: its packet among the boundaries [b_lo, b_hi) of the tile, the byte, and whether a
// packet starts with it
__device__ __forceinline__ unsigned fr_fetch(const FrameArgs& a, long b_lo, long b_hi, u64 G, long& p, bool& start) {
    p = fr_upper(a.pb, b_lo, b_hi, G) - 1;     // (empty packets share their pb with the next one: the last of them holds G)
    const u64 j = G - a.pb[p], len = a.pb[p + 1] - a.pb[p] - (a.fcs ? 2 : 0);
    start = j == 0;
    return j < len ? a.bytes[a.starts[p] + j] : (a.crc[p] >> (8 * (unsigned)(j - len))) & 0xffu;      // low byte first
}
// the boundaries of the tile that begins at byte tb0, by thread 0, for everyone
__device__ __forceinline__ void fr_bounds(const FrameArgs& a, long tile, long* s_b) {
    if (threadIdx.x == 0) {
        const u64 tb0 = (u64)tile * FR_TB;
        s_b[0] = fr_lower(a.pb, 0, a.P + 1, tb0);
        s_b[1] = tile == a.ntiles - 1 ? a.P + 1 : fr_lower(a.pb, 0, a.P + 1, tb0 + FR_TB);      // the last tile: those at nbytes too
    }
    __syncthreads();
}

__global__ __launch_bounds__(FR_B) void k_frame_sum(FrameArgs a) {
    __shared__ long s_b[2];
    __shared__ StuffSum s_w[FR_B / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        fr_bounds(a, tile, s_b);
        const long b_lo = s_b[0], b_hi = s_b[1];
        StuffSum v = stuff_none();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long G = tile * FR_TB + 2 * tid + h;
            if (G < a.nbytes) {
                long p;
                bool start;
                const unsigned byte = fr_fetch(a, b_lo, b_hi, (u64)G, p, start);
                a.lb[G] = (unsigned char)byte;
                if (start) v = stuff_combine(v, stuff_start());
                v = stuff_combine(v, stuff_byte(byte));
            }
        }
        v = fr_wave_scan(v, lane);
        if (lane == 63) s_w[wave] = v;
        __syncthreads();
        if (tid == 0) {
            StuffSum t = s_w[0];
            for (int q = 1; q < FR_B / 64; ++q) t = stuff_combine(t, s_w[q]);
            reinterpret_cast<StuffSum*>(a.sums)[tile] = t;
        }
        __syncthreads();                      // the next tile overwrites s_b and s_w
    }
}

__global__ __launch_bounds__(FR_SB) void k_frame_scan(FrameArgs a) {
    __shared__ StuffSum s_w[FR_SB / 64];
    __shared__ StuffSum s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const StuffSum* sums = reinterpret_cast<const StuffSum*>(a.sums);
    if (tid == 0) s_run = stuff_carry(0);     // the counter is 0 in front of the first packet
    __syncthreads();
    for (long c0 = 0; c0 < a.ntiles; c0 += FR_SB) {
        const long t = c0 + tid;
        const StuffSum mine = t < a.ntiles ? sums[t] : stuff_none();
        const StuffSum inc = fr_wave_scan(mine, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        StuffSum before = s_run;
        for (int q = 0; q < wave; ++q) before = stuff_combine(before, s_w[q]);
        StuffSum prev = fr_shfl_up(inc, 1);
        if (lane == 0) prev = stuff_none();
        const StuffSum ex = stuff_combine(before, prev);              // (holds a break: trail and stuffs are the counter and C)
        if (t < a.ntiles) { a.tin[2 * t] = ex.trail; a.tin[2 * t + 1] = ex.stuffs; }
        __syncthreads();                      // everyone has read s_run and s_w
        if (tid == FR_SB - 1) s_run = stuff_combine(before, inc);
        __syncthreads();
    }
}

__global__ __launch_bounds__(FR_B) void k_frame_emit(FrameArgs a) {
    __shared__ long s_b[2];
    __shared__ StuffSum s_w[FR_B / 64];
    __shared__ unsigned s_cnt[FR_TB + 1];     // C at every byte of the tile and behind its last
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long nbits = 8 * a.nbytes;
    for (long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        fr_bounds(a, tile, s_b);
        const long b_lo = s_b[0], b_hi = s_b[1];
        const long tb0 = tile * FR_TB;
        unsigned byte[2] = {0, 0};
        long pk[2] = {0, 0};
        bool start[2] = {false, false};
        StuffSum v = stuff_none();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long G = tb0 + 2 * tid + h;
            if (G < a.nbytes) {
                pk[h] = fr_upper(a.pb, b_lo, b_hi, (u64)G) - 1;
                start[h] = a.pb[pk[h]] == (u64)G;
                byte[h] = a.lb[G];
                if (start[h]) v = stuff_combine(v, stuff_start());
                v = stuff_combine(v, stuff_byte(byte[h]));
            }
        }
        const StuffSum inc = fr_wave_scan(v, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        StuffSum before = StuffSum{1u, 0u, a.tin[2 * tile], a.tin[2 * tile + 1]};
        for (int q = 0; q < wave; ++q) before = stuff_combine(before, s_w[q]);
        StuffSum prev = fr_shfl_up(inc, 1);
        if (lane == 0) prev = stuff_none();
        const StuffSum ex = stuff_combine(before, prev);
        // hdlc_encode's loop over the thread's 16 bits, from the counter and the C in front of them
        unsigned ones = ex.trail, cnt = ex.stuffs;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            s_cnt[2 * tid + h] = cnt;
            const long g0 = 8 * (tb0 + 2 * tid + h);
            if (g0 < nbits) {
                if (start[h]) ones = 0;
                const long base = 320 * pk[h] + 160 + g0;
                for (int i = 0; i < 8; ++i) {
                    const unsigned b = byte[h] >> i & 1u;
                    const long pos = base + i + (long)cnt;
                    if (pos < a.cap) a.pre[pos] = (unsigned char)b;            // (always: the bound holds for every payload)
                    if (b) {
                        if (++ones == 5) { ones = 0; ++cnt; if (pos + 1 < a.cap) a.pre[pos + 1] = 0; }
                    } else {
                        ones = 0;
                    }
                }
            }
        }
        if (tid == FR_B - 1) s_cnt[FR_TB] = cnt;
        __syncthreads();
        // the boundaries of the tile: 320 flag bits around each (160 at the two ends of the batch)
        const long nflag = (b_hi - b_lo) * 320;
        for (long idx = tid; idx < nflag; idx += FR_B) {
            const long b = b_lo + idx / 320;
            const int k = (int)(idx % 320);
            const u64 gb = a.pb[b];
            const u64 o = gb - (u64)tb0;                                  // 0 .. FR_TB: the bytes of this tile, or nbytes behind the last
            const unsigned C = s_cnt[o < (u64)FR_TB ? o : (u64)FR_TB];
            if (k == 0) a.cb[b] = C;
            if ((k < 160 && b == 0) || (k >= 160 && b == a.P)) continue;
            const long pos = 320 * b - 160 + 8 * (long)gb + (long)C + k;
            if (pos < a.cap) a.pre[pos] = (unsigned char)(0x7eu >> (k & 7) & 1u);
        }
        if (tile == a.ntiles - 1 && tid == 0) *a.total = (u64)(320 * a.P + nbits) + s_cnt[FR_TB];
        __syncthreads();                      // the next tile overwrites the shared arrays
    }
}

void launch_frame(const FrameArgs& a, hipStream_t s) {
    if (a.P <= 0) return;
    if (a.fcs) {
        const unsigned gc = tiles_grid((a.nchunks + FR_B - 1) / FR_B);
        hipLaunchKernelGGL(k_frame_crc_chunks, dim3(gc), dim3(FR_B), 0, s, a);
        const unsigned gf = tiles_grid((a.P + FR_B / 64 - 1) / (FR_B / 64));
        hipLaunchKernelGGL(k_frame_crc_fold, dim3(gf), dim3(FR_B), 0, s, a);
    }
    const unsigned gt = tiles_grid(a.ntiles);
    hipLaunchKernelGGL(k_frame_sum, dim3(gt), dim3(FR_B), 0, s, a);
    hipLaunchKernelGGL(k_frame_scan, dim3(1), dim3(FR_SB), 0, s, a);
    hipLaunchKernelGGL(k_frame_emit, dim3(gt), dim3(FR_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

// ---- the line coder ---------------------------------------------------------------------------------------------------------------------
// One tile of cnt bits (1 .. LINE_T) of `in` with the state st in front of it; every thread of the workgroup calls it.  Returns
// the state behind the tile's last bit; *res: the LINE_W output words, in s_a or s_b.
__device__ __forceinline__ unsigned line_tile(const unsigned char* __restrict__ in, int cnt, int mode, unsigned st, u64* s_a, u64* s_b,
                                              unsigned* s_misc, u64** res) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int g = i * FR_B + tid;
        const u64 b = __ballot(g < cnt && (in[g < cnt ? g : 0] & 1u) != 0);
        if (lane == 0) s_a[i * (FR_B / 64) + wave] = b;
    }
    if (tid < 2) s_misc[tid] = 0;
    __syncthreads();
    u64 *a = s_a, *b = s_b;
    if (mode & LINE_SCR) {
        if (tid == 0) a[0] ^= line_inject(st);
        __syncthreads();
        for (int k = 0; k < LINE_K; ++k) {     // s = in / (1 + x^12 + x^17) modulo x^LINE_T, as a product of LINE_K trinomials
            if (tid < LINE_W) b[tid] = a[tid] ^ line_delay(a, tid, 12 << k) ^ line_delay(a, tid, 17 << k);
            __syncthreads();
            u64* t = a; a = b; b = t;
        }
        if (tid == 0) {                        // the 17 bits of (register ++ s) behind bit cnt
            unsigned reg = 0;
            for (int k = 0; k < 17; ++k) {
                const int idx = cnt + k;
                const unsigned bit = idx < 17 ? st >> idx & 1u : (unsigned)(a[(idx - 17) >> 6] >> ((idx - 17) & 63)) & 1u;
                reg |= bit << k;
            }
            s_misc[0] = reg;
        }
        if (tid < LINE_W) b[tid] = line_delay(a, tid, 17) | (tid == 0 ? (u64)(st & 0x1ffffu) : 0ull);       // out[n] = s[n - 17]
        __syncthreads();
        u64* t = a; a = b; b = t;
    }
    if (mode & LINE_NRZI) {
        if (tid < LINE_W) {                    // (wave 0, whole) the level behind bit n: the parity of the zeros up to it
            u64 x = ~a[tid];
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
            const u64 m = __ballot((x >> 63) != 0);
            const unsigned lvl = (st >> 17 & 1u) ^ ((unsigned)__popcll(m & ((1ull << tid) - 1ull)) & 1u);
            a[tid] = lvl ? ~x : x;
        }
        __syncthreads();
        if (tid == 0) s_misc[1] = (unsigned)(a[(cnt - 1) >> 6] >> ((cnt - 1) & 63)) & 1u;
    }
    __syncthreads();
    *res = a;
    return s_misc[0] | s_misc[1] << 17;
}
__device__ __forceinline__ long line_n(const LineArgs& a) {
    if (!a.n_dev) return a.max_n;
    const u64 n = *a.n_dev;
    return n < (u64)a.max_n ? (long)n : a.max_n;
}

__global__ __launch_bounds__(FR_B) void k_line_z(LineArgs a) {
    __shared__ u64 s_a[LINE_W], s_b[LINE_W];
    __shared__ unsigned s_misc[2];
    const long n = line_n(a), nfull = (n + LINE_T - 1) / LINE_T - 1;          // the tiles in front of the last one
    for (long tile = blockIdx.x; tile < nfull; tile += gridDim.x) {
        u64* res;
        const unsigned z = line_tile(a.in + tile * LINE_T, LINE_T, a.mode, 0u, s_a, s_b, s_misc, &res);
        if (threadIdx.x == 0) a.z[tile] = z;
        __syncthreads();                      // the next tile overwrites the shared arrays
    }
}

__global__ __launch_bounds__(FR_SB) void k_line_scan(LineArgs a) {
    __shared__ unsigned s_pw[LINE_NP * LINE_NS];
    __shared__ unsigned s_w[FR_SB / 64];
    __shared__ unsigned s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < LINE_NP * LINE_NS; i += FR_SB) s_pw[i] = a.pw[i];
    if (tid == 0) { s_run = *a.st_in; a.carry[0] = s_run; }
    __syncthreads();
    const long n = line_n(a), m = (n + LINE_T - 1) / LINE_T - 1;
    for (long c0 = 0; c0 < m; c0 += FR_SB) {
        const long i = c0 + tid;
        unsigned v = i < m ? a.z[i] : 0u;      // after round r: the response of the 2^(r+1) tiles that end with this one
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const unsigned u = __shfl_up(v, 1 << r, 64);
            if (lane >= (1 << r)) v ^= line_matvec(s_pw + r * LINE_NS, u);
        }
        if (lane == 63) s_w[wave] = v;
        __syncthreads();
        unsigned x = 0;                         // the waves in front of this one
        for (int q = 0; q < wave; ++q) x = line_matvec(s_pw + 6 * LINE_NS, x) ^ s_w[q];
        const unsigned c = line_pow_apply(s_pw, (u64)tid + 1, s_run) ^ line_pow_apply(s_pw, (u64)lane + 1, x) ^ v;
        if (i < m) a.carry[i + 1] = c;
        __syncthreads();                      // everyone has read s_run and s_w
        if (tid == FR_SB - 1) s_run = c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(FR_B) void k_line_emit(LineArgs a) {
    __shared__ u64 s_a[LINE_W], s_b[LINE_W];
    __shared__ unsigned s_misc[2];
    const int tid = threadIdx.x;
    const long n = line_n(a), ntiles = (n + LINE_T - 1) / LINE_T;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long t0 = tile * LINE_T;
        const int cnt = (int)(n - t0 < LINE_T ? n - t0 : LINE_T);
        u64* res;
        const unsigned st = line_tile(a.in + t0, cnt, a.mode, a.mode ? a.carry[tile] : 0u, s_a, s_b, s_misc, &res);
        if (a.mode && tile == ntiles - 1 && tid == 0) *a.st_out = st;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = i * FR_B + tid;
            if (j < cnt) {
                const unsigned bit = (unsigned)(res[j >> 6] >> (j & 63)) & 1u;
                if (a.out_f32) static_cast<float*>(a.out)[t0 + j] = bit ? a.hi : a.lo;
                else static_cast<unsigned char*>(a.out)[t0 + j] = (unsigned char)bit;
            }
        }
        __syncthreads();                      // the next tile overwrites the shared arrays
    }
}

void launch_line(const LineArgs& a, hipStream_t s) {
    if (a.max_n <= 0) return;
    const long ntiles = (a.max_n + LINE_T - 1) / LINE_T;
    const unsigned grid = tiles_grid(ntiles);
    if (a.mode) {
        hipLaunchKernelGGL(k_line_z, dim3(grid), dim3(FR_B), 0, s, a);
        hipLaunchKernelGGL(k_line_scan, dim3(1), dim3(FR_SB), 0, s, a);
    }
    hipLaunchKernelGGL(k_line_emit, dim3(grid), dim3(FR_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
