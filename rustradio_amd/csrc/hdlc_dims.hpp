// hdlc_dims.hpp — the tile sizes of the HDLC deframer's kernels, apart from kernels.hpp so that hdlc_host.hpp (no HIP) plans with them.
#pragma once
namespace rr {
constexpr int HDLC_T = 4096;                  // virtual bits of one tile
constexpr int HDLC_GB = 256;                  // gaps of one block of the map scan
}  // namespace rr
