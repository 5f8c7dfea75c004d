// kernels_hdlc.hip — the end of the packet receivers (examples/ax25-9600-rx.rs, ax25-1200-rx.rs, bell202.rs, g3ruh.rs):
//   HdlcDeframer (src/hdlc_deframer.rs:123-232, find_right_crc :41-71, calc_crc :309-315)
// over the next n bits of a stream (the arithmetic is hdlc_core.hpp's, the formulation deframe_events of
// tests/hdlc_model.py).  The bits of a push stand behind what the stream so far left on the device — 8 halo bits, then the raw
// bits of the gap still open — as one VIRTUAL stream, cut into tiles of HDLC_T bits:
//   k_hdlc_mark      the tile's bits as words, and its flag ends, aborts and stuffed zeros as masks; the flag ends of the tile
//   k_hdlc_offs      ONE workgroup: the flag ends in front of every tile
//   k_hdlc_ends      the flag ends in stream order
//   k_hdlc_gap       one thread per gap between two flag ends: its map over {S, U, U3}; the maps of HDLC_GB gaps scanned
//   k_hdlc_resolve   ONE workgroup: the machine in front of every block of gaps, from the carried one
//   k_hdlc_emit      one wave per gap that is a frame: destuffed, packed, checked, repaired, stored at byte floor((s + 1) / 8)
//   k_hdlc_carry     ONE workgroup: what the next push starts from
// No workgroup waits on another; the grids depend on the host's bound of the virtual length alone.  Gaps are disjoint and a
// frame has at most (f - s - 8) / 8 bytes, so every arena byte has one writer; only the record list and the three counters are
// appended atomically.  The bodies are hdlc_body.hpp's (kernels_hdlcrx.hip runs the same ones over N streams); the kernels here
// give them the host's view of the one stream, its bits as bytes, and rr_hdlc_frame records.
#include "hdlc_body.hpp"

namespace rr {

static_assert(sizeof(HdlcRec) == 24, "HdlcRec is rr_hdlc_frame");

__global__ __launch_bounds__(HD_B) void k_hdlc_mark(HdlcArgs a) { hd_mark_body(a, HdlcByteSrc{}, blockIdx.x == 0, blockIdx.x == 0); }
__global__ __launch_bounds__(HD_SB) void k_hdlc_offs(HdlcArgs a) { hd_offs_body(a); }
__global__ __launch_bounds__(64) void k_hdlc_ends(HdlcArgs a) { hd_ends_body(a); }
__global__ __launch_bounds__(HDLC_GB) void k_hdlc_gap(HdlcArgs a) { hd_gap_body(a); }
__global__ __launch_bounds__(HD_SB) void k_hdlc_resolve(HdlcArgs a) { hd_resolve_body(a); }
__global__ __launch_bounds__(HD_B) void k_hdlc_emit(HdlcArgs a) { hd_emit_body(a, HdlcRecSink{}); }
__global__ __launch_bounds__(HD_B) void k_hdlc_carry(HdlcArgs a) { hd_carry_body(a); }

void launch_hdlc(const HdlcArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    const unsigned gt = tiles_grid(a.ntiles);
    const unsigned gg = tiles_grid((a.ends_cap + HDLC_GB - 1) / HDLC_GB);
    const unsigned ge = tiles_grid((a.ends_cap + HD_B / 64 - 1) / (HD_B / 64));
    hipLaunchKernelGGL(k_hdlc_mark, dim3(gt), dim3(HD_B), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_offs, dim3(1), dim3(HD_SB), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_ends, dim3(gt), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_gap, dim3(gg), dim3(HDLC_GB), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_resolve, dim3(1), dim3(HD_SB), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_emit, dim3(ge), dim3(HD_B), 0, s, a);
    hipLaunchKernelGGL(k_hdlc_carry, dim3(1), dim3(HD_B), 0, s, a);
    RR_HIP(hipGetLastError());
}

}  // namespace rr
