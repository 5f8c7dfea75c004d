// kernels_bits.hip — the bit-level sync blocks behind every data receiver of the reference's examples, one tile kernel:
//   BinarySlicer (src/binary_slicer.rs:17-19) -> XorConst(1) -> NrziDecode (src/nrzi.rs:36-41) ->
//   Descrambler (src/descrambler.rs:34-39) -> CorrelateAccessCodeTag (src/correlate_access_code.rs:93-118)
// as wired in examples/ax25-9600-rx.rs:195-204 and examples/il2p-1200-rx.rs:118-126.  Every stage is optional and all of
// them are feed-forward: a bit after stage k is an XOR of a few EARLIER bits of stage k-1 (NRZI: 1 back; the descrambler:
// 1..64 back; the correlator looks at 64).  So a workgroup packs its tile of BITS_T samples into 64-bit words in LDS,
// puts the 128 bits before the tile in front of them and runs the stages as shifts and XORs on words:
//   R  the sliced (and inverted) input bits          r[n]
//   D  after NRZI                                     d[n] = 1 ^ r[n] ^ r[n-1]
//   S  after the descrambler                          s[n] = d[n] ^ XOR_delta d[n - delta], delta in 1..64
//   correlator: popcount((64 bits of S ending at n) >> (64 - L) ^ code) per position n
// The 128 bits in front of a tile that starts inside the window are recomputed from the 128 input samples before it; only
// the tile at the window's start takes them from the state the handle carries (the last r, the last 64 d, the last 64 s, the
// count of bits seen).  No workgroup waits on another one and there is one launch per call.
#include "kernels.hpp"
#include "packet_common.hpp"

namespace rr {

constexpr int BITS_B = 256;                   // threads of a workgroup
constexpr int BITS_PER = 16;                  // consecutive samples of one thread: 16 B of u8, four float4
constexpr int BITS_W = BITS_T / 64;           // words of a tile
constexpr int BITS_HW = 2;                    // words of history in front of them
constexpr int BITS_NW = BITS_HW + BITS_W;
static_assert(BITS_B * BITS_PER == BITS_T && BITS_T % 64 == 0 && BITS_T >= 128, "one tile = 16 samples per thread");
static_assert(BITS_NW <= BITS_B, "the word stages run one word per thread");

typedef unsigned long long u64;

// four bytes holding 0 / 1 in their lowest bit -> four bits, byte k to bit k; and back (32-bit multiplies, no carries)
__device__ __forceinline__ unsigned bits_pack4(unsigned x) { return ((x & 0x01010101u) * 0x01020408u) >> 24 & 0xfu; }
__device__ __forceinline__ unsigned bits_spread4(unsigned b) { return ((b & 0xfu) * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ unsigned bits_one(float v) { return v > 0.0f ? 1u : 0u; }          // binary_slicer.rs:17-19: NaN, -0.0 -> 0
__device__ __forceinline__ unsigned bits_one(unsigned char v) { return v & 1u; }

// 16 consecutive samples at p (16-byte aligned) -> 16 bits
__device__ __forceinline__ unsigned bits_load16(const float* p) {
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        m |= (bits_one(v.x) | bits_one(v.y) << 1 | bits_one(v.z) << 2 | bits_one(v.w) << 3) << (4 * q);
    }
    return m;
}
__device__ __forceinline__ unsigned bits_load16(const unsigned char* p) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    return bits_pack4(v.x) | bits_pack4(v.y) << 4 | bits_pack4(v.z) << 8 | bits_pack4(v.w) << 12;
}
// the samples lo <= n < hi among the 16 that start at n0, one guarded load each
template <class T> __device__ __forceinline__ unsigned bits_load_guarded(const T* in, long n0, long lo, long hi) {
    unsigned m = 0;
    for (int i = 0; i < BITS_PER; ++i)
        if (n0 + i >= lo && n0 + i < hi) m |= bits_one(in[n0 + i]) << i;
    return m;
}

// word w of the bit array kept as 16-bit pieces
__device__ __forceinline__ u64 bits_word(const unsigned short* a, int w) {
    return (u64)a[4 * w] | (u64)a[4 * w + 1] << 16 | (u64)a[4 * w + 2] << 32 | (u64)a[4 * w + 3] << 48;
}
// the 64 bits of A that end at bit position p (p >= 63): bit 63 of the result is bit p
__device__ __forceinline__ u64 bits_win64(const u64* A, int p) {
    const int b = p - 63, wi = b >> 6, off = b & 63;
    return off ? (A[wi] >> off) | (A[wi + 1] << (64 - off)) : A[wi];
}

// VIN / VOUT: the window's input / output pointer is 16-byte aligned, so a thread moves its 16 samples in 16-byte accesses;
// otherwise the whole window takes the guarded path of one sample per lane and step (coalesced, narrow).
template <class SRC, bool VIN, bool VOUT>
__global__ __launch_bounds__(BITS_B) void k_bits(const SRC* __restrict__ in, unsigned char* __restrict__ out, long n, BitsCfg c,
                                                 const u64* __restrict__ st_in, u64* __restrict__ st_out, unsigned* __restrict__ tilecnt,
                                                 u64* __restrict__ list) {
    __shared__ unsigned short s_r[BITS_NW * 4];
    __shared__ u64 s_d[BITS_NW], s_s[BITS_NW];
    __shared__ int s_cnt[BITS_B / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long ntiles = (n + BITS_T - 1) / BITS_T;
    const unsigned inv16 = c.invert ? 0xffffu : 0u;
    const u64 seen0 = st_in[BITS_ST_SEEN], dhist0 = st_in[BITS_ST_DHIST], shist0 = st_in[BITS_ST_SHIST];
    const long first = (long)c.L - 1 - (long)seen0;           // tags from this sample of the window on: L bits seen
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long t0 = tile * BITS_T;
        // ---- R: the tile's bits, 16 per thread, and the 128 before them ----
        if (VIN) {
            const long n0 = t0 + (long)tid * BITS_PER;
            unsigned m = 0;
            if (n0 + BITS_PER <= n) m = bits_load16(in + n0);
            else if (n0 < n) m = bits_load_guarded(in, n0, 0, n);
            s_r[BITS_HW * 4 + tid] = (unsigned short)(m ^ inv16);
            if (t0 > 0 && tid < BITS_HW * 4) s_r[tid] = (unsigned short)(bits_load16(in + t0 - 64 * BITS_HW + tid * BITS_PER) ^ inv16);
        } else {
            for (int i = 0; i < BITS_PER; ++i) {
                const long g = t0 + i * BITS_B + tid;
                const u64 b = __ballot(g < n && (bits_one(in[g < n ? g : 0]) ^ (unsigned)c.invert) != 0);
                if (lane < 4) s_r[(BITS_HW + i * (BITS_B / 64) + wave) * 4 + lane] = (unsigned short)(b >> (16 * lane));
            }
            if (t0 > 0 && tid < 64 * BITS_HW) {               // (two whole waves)
                const u64 b = __ballot((bits_one(in[t0 - 64 * BITS_HW + tid]) ^ (unsigned)c.invert) != 0);
                if (lane < 4) s_r[wave * 4 + lane] = (unsigned short)(b >> (16 * lane));
            }
        }
        if (t0 == 0 && tid < BITS_HW * 4) s_r[tid] = tid == BITS_HW * 4 - 1 ? (unsigned short)(st_in[BITS_ST_RLAST] << 15) : 0;
        __syncthreads();
        // ---- D and S, one word per thread: NRZI on the word and on the one before it, then the descrambler,
        //      s[n] = d[n] ^ XOR d[n - delta] over the set bits (delta - 1) of dmask.  The history words of the window's first
        //      tile are the carried ones.  (Word 0 of D and S and bit 0 of word 1 are never looked at: nothing reaches back
        //      more than 127 bits.) ----
        if (tid < BITS_NW) {
            const u64 r0 = bits_word(s_r, tid), r1 = tid ? bits_word(s_r, tid - 1) : 0ull, r2 = tid > 1 ? bits_word(s_r, tid - 2) : 0ull;
            u64 cur = c.nrzi ? ~(r0 ^ (r0 << 1 | r1 >> 63)) : r0;
            u64 prev = c.nrzi ? ~(r1 ^ (r1 << 1 | r2 >> 63)) : r1;
            if (t0 == 0 && tid <= BITS_HW) {
                cur = tid == BITS_HW - 1 ? dhist0 : tid < BITS_HW ? 0ull : cur;
                prev = tid == BITS_HW ? dhist0 : 0ull;
            }
            u64 acc = cur;
            for (u64 dm = c.dmask; dm; dm &= dm - 1) {
                const int delta = __ffsll(dm);
                acc ^= delta == 64 ? prev : (cur << delta | prev >> (64 - delta));
            }
            if (t0 == 0 && tid < BITS_HW) acc = tid == BITS_HW - 1 ? shist0 : 0ull;
            s_d[tid] = cur;
            s_s[tid] = acc;
        }
        __syncthreads();
        // ---- out: 16 bytes per thread ----
        const long n0 = t0 + (long)tid * BITS_PER;
        const unsigned m = (unsigned)(s_s[BITS_HW + tid / 4] >> (16 * (tid & 3))) & 0xffffu;      // the thread's 16 output bits
        if (VOUT) {
            if (n0 + BITS_PER <= n) {
                *reinterpret_cast<uint4*>(out + n0) = make_uint4(bits_spread4(m), bits_spread4(m >> 4), bits_spread4(m >> 8), bits_spread4(m >> 12));
            } else {
                for (int i = 0; i < BITS_PER; ++i)
                    if (n0 + i < n) out[n0 + i] = (unsigned char)((m >> i) & 1u);
            }
        } else {
            for (int i = 0; i < BITS_PER; ++i) {
                const int j = i * BITS_B + tid;
                if (t0 + j < n) out[t0 + j] = (unsigned char)((s_s[BITS_HW + (j >> 6)] >> (j & 63)) & 1ull);
            }
        }
        // ---- the correlator: the L bits of S that end at each of the thread's 16 positions against the code ----
        const int p0 = 64 * BITS_HW + tid * BITS_PER;         // bit position of the thread's first sample
        if (c.L) {
            // b0: the 64 bits of S that end at the thread's first sample (one funnel shift); its later samples are its own
            // output bits, so every further window is b0 and m shifted by a constant.  Up to 32 bits of code: 32-bit words.
            const u64 b0 = bits_win64(s_s, p0), later = (u64)(m >> 1);
            unsigned hits = 0;
            if (c.L <= 32) {
                const u64 w = b0 >> 32 | later << 32;
                const unsigned code = (unsigned)c.code;
                const int shr = 32 - c.L;
#pragma unroll
                for (int i = 0; i < BITS_PER; ++i)
                    if ((unsigned)__popc(((unsigned)(w >> i) >> shr) ^ code) <= c.allowed) hits |= 1u << i;
            } else {
                const int shr = 64 - c.L;
#pragma unroll
                for (int i = 0; i < BITS_PER; ++i) {
                    const u64 x = i ? b0 >> i | later << (64 - i) : b0;
                    if ((unsigned)__popcll((x >> shr) ^ c.code) <= c.allowed) hits |= 1u << i;
                }
            }
            // ... of the samples inside the window, once L bits of the stream have been seen
            const long lo = first - n0, hi = n - n0;
            const unsigned keep = (hi >= BITS_PER ? 0xffffu : hi <= 0 ? 0u : (1u << hi) - 1u) &
                                  (lo <= 0 ? 0xffffu : lo >= BITS_PER ? 0u : 0xffffu << lo);
            hits &= keep;
            // Slots: tile t owns list[t BITS_T ..) and tilecnt[t], so nothing is asked of another workgroup and no atomic is
            // needed; the threads' counts are scanned over the wave, the waves' over LDS, and the entries of a tile land in
            // ascending order.  k_bits_tag_offsets / k_bits_tag_gather close the gaps when the host asks for the tags.
            const int cnt = __popc(hits);
            int inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o, 64);
                if (lane >= o) inc += u;
            }
            if (lane == 63) s_cnt[wave] = inc;
            __syncthreads();
            int tot = 0, before = 0;                                  // (every thread sums the four wave totals itself)
#pragma unroll
            for (int w = 0; w < BITS_B / 64; ++w) { const int v = s_cnt[w]; if (w < wave) before += v; tot += v; }
            if (tid == 0) tilecnt[tile] = (unsigned)tot;
            u64* dst = list + t0 + before + inc - cnt;
            for (unsigned h = hits; h; h &= h - 1) {                  // (rare: the differences are counted again here)
                const int i = __ffs(h) - 1;
                const u64 x = i ? b0 >> i | later << (64 - i) : b0;
                *dst++ = (u64)(n0 + i) << 8 | (u64)__popcll((x >> (64 - c.L)) ^ c.code);
            }
        }
        // ---- the thread that holds the window's last sample writes what the next call starts from ----
        if (n - 1 >= n0 && n - 1 < n0 + BITS_PER) {
            const int p = p0 + (int)(n - 1 - n0);
            st_out[BITS_ST_RLAST] = (bits_word(s_r, p >> 6) >> (p & 63)) & 1ull;
            st_out[BITS_ST_DHIST] = bits_win64(s_d, p);
            st_out[BITS_ST_SHIST] = bits_win64(s_s, p);
            st_out[BITS_ST_SEEN] = seen0 + (u64)n < 64ull ? seen0 + (u64)n : 64ull;       // saturating
        }
        __syncthreads();                      // the next tile overwrites the three arrays and s_cnt
    }
}

// The tags of a call, gathered: offs[t] = tilecnt[0] + .. + tilecnt[t-1] and *total, by ONE workgroup (a window of 1e8 samples
// has 24,415 tiles); then one workgroup per tile moves its entries to out[offs[t] ..).  Tiles and the entries inside one are
// in ascending order, so `out` is sorted by position.  Both run only when the host asks for the tags (rr_bit_tags).
constexpr int BITS_OB = 1024;
__global__ __launch_bounds__(BITS_OB) void k_bits_tag_offsets(const unsigned* __restrict__ tilecnt, long ntiles, u64* __restrict__ offs,
                                                              u64* __restrict__ total) {
    __shared__ u64 s_w[BITS_OB / 64];
    __shared__ u64 s_run;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (long c0 = 0; c0 < ntiles; c0 += BITS_OB) {
        const long t = c0 + tid;
        const u64 v = t < ntiles ? tilecnt[t] : 0ull;
        u64 inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        u64 before = s_run;
        for (int w = 0; w < wave; ++w) before += s_w[w];
        if (t < ntiles) offs[t] = before + inc - v;
        __syncthreads();                      // everyone has read s_run and s_w
        if (tid == BITS_OB - 1) s_run = before + inc;
        __syncthreads();
    }
    if (tid == 0) *total = s_run;
}
__global__ __launch_bounds__(BITS_B) void k_bits_tag_gather(const unsigned* __restrict__ tilecnt, const u64* __restrict__ offs,
                                                            const u64* __restrict__ list, long ntiles, u64* __restrict__ out) {
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned cnt = tilecnt[t];
        const u64* src = list + t * BITS_T;
        u64* dst = out + offs[t];
        for (unsigned j = threadIdx.x; j < cnt; j += BITS_B) dst[j] = src[j];
    }
}
void launch_bits_tag_offsets(const unsigned* tilecnt, long ntiles, u64* offs, u64* total, hipStream_t s) {
    hipLaunchKernelGGL(k_bits_tag_offsets, dim3(1), dim3(BITS_OB), 0, s, tilecnt, ntiles, offs, total);
    RR_HIP(hipGetLastError());
}
void launch_bits_tag_gather(const unsigned* tilecnt, const u64* offs, const u64* list, long ntiles, u64* out, hipStream_t s) {
    const unsigned grid = tiles_grid(ntiles);
    hipLaunchKernelGGL(k_bits_tag_gather, dim3(grid), dim3(BITS_B), 0, s, tilecnt, offs, list, ntiles, out);
    RR_HIP(hipGetLastError());
}

template <class SRC>
static void bits_launch(const SRC* in, unsigned char* out, long n, const BitsCfg& c, const u64* st_in, u64* st_out, unsigned* tilecnt,
                        u64* list, hipStream_t s) {
    if (n <= 0) return;
    const long ntiles = (n + BITS_T - 1) / BITS_T;
    const unsigned grid = tiles_grid(ntiles);
    const bool vin = reinterpret_cast<uintptr_t>(in) % 16 == 0, vout = reinterpret_cast<uintptr_t>(out) % 16 == 0;
#define RR_BITS_GO(VI, VO) hipLaunchKernelGGL((k_bits<SRC, VI, VO>), dim3(grid), dim3(BITS_B), 0, s, in, out, n, c, st_in, st_out, tilecnt, list)
    if (vin && vout) RR_BITS_GO(true, true);
    else if (vin) RR_BITS_GO(true, false);
    else if (vout) RR_BITS_GO(false, true);
    else RR_BITS_GO(false, false);
#undef RR_BITS_GO
    RR_HIP(hipGetLastError());
}

void launch_bits_f32(const float* in, unsigned char* out, long n, const BitsCfg& c, const u64* st_in, u64* st_out, unsigned* tilecnt,
                     u64* list, hipStream_t s) {
    bits_launch<float>(in, out, n, c, st_in, st_out, tilecnt, list, s);
}
void launch_bits_u8(const unsigned char* in, unsigned char* out, long n, const BitsCfg& c, const u64* st_in, u64* st_out, unsigned* tilecnt,
                    u64* list, hipStream_t s) {
    bits_launch<unsigned char>(in, out, n, c, st_in, st_out, tilecnt, list, s);
}

}  // namespace rr
