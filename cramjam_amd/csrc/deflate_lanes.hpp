// deflate_lanes.hpp — what deflate.hip and deflate_encode.hip share: the device accessors that deflate_wave.hpp and
// deflate_enc_wave.hpp are written against (the lists at the top of those two files; tests/hostsim has bounds-checked stand-ins of
// its own for the host builds), and the check of a cj_deflate_wrap.  Each of the two files adds what only its own text names
// (the decoder LaneBytes; the encoder LaneU32 / LaneU64, lane_excl_add, in_ld8, out_st8 / out_st32, rec_ld).  Not part of the C-ABI.
#pragma once
#include "cj_stage.hpp"

namespace cj {

#define CJ_LANES(lane) for (uint32_t lane = lane_id(); lane < 64u; lane += 64u)

__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) { return uni(*p); }
__device__ __forceinline__ uint32_t lds_ld8(const uint8_t* p) { return uni((uint32_t)*p); }
__device__ __forceinline__ uint32_t out_ld8(const uint8_t* p) { return uni((uint32_t)*p); }
__device__ __forceinline__ void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_xor(uint32_t* p, uint32_t v) { atomicXor(p, v); }
__device__ __forceinline__ void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }

inline bool deflate_wrap_ok(int wrap) { return wrap == CJ_DEFLATE_RAW || wrap == CJ_DEFLATE_ZLIB || wrap == CJ_DEFLATE_GZIP; }

}  // namespace cj
