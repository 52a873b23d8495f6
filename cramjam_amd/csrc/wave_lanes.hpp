// wave_lanes.hpp — the device implementation of the wave-decoder contract: the accessors that the *_wave.hpp
// headers name and, with cj_common.hpp's InWindow (opened by wave_window.hpp's window_open), wave_copy, wave_match_copy and wave_order,
// everything they name.  The host
// implementation, every access checked against registered ranges, is tests/hostsim/sim_wave.hpp.  This is the one place that says
// what each accessor means:
//     CJ_LANES(lane)            the body that follows runs once per lane (here: for this lane; the host: a loop over 0..63).  A body
//                               never reads what another lane writes in the SAME body; wave_order() separates bodies
//     lds_ld(p), lds_ld8(p)     a wave-uniform 32-bit / 8-bit read of the wavefront's LDS
//     lds_add / lds_xor / lds_or(p, v)     lane-wise read-modify-write of an LDS word
//     in_ld8(p), in_ld32(p)     a lane's own read of one byte / an (unaligned) dword of the input
//     out_ld8(p)                a wave-uniform read of one byte of the output written so far;  out_rd32(p): a lane's own dword of it
//     out_st8(p, v), out_st32(p, v)        a lane's own store of a byte / an (unaligned) dword of the output
//     slot_st8(p, v)            a lane's own store into the wavefront's scratch slot, which wave_copy may read back
//     LaneBytes                 put(k, byte): lane k keeps a byte; flush(dst, n): lanes 0..n-1 store theirs to dst[lane], n <= 64
//     LaneU32, LaneU64          a value per lane: v[lane] inside a CJ_LANES body
//     lane_excl_add(v, before)  before[lane] = the sum of v below that lane; returns the sum of all 64 (wave-uniform)
// (rec_ld, the encoder's read of a sequence record, needs the complete DfeRec and is cj_rec_encode.hpp's.)  Not part of the C-ABI.
#pragma once
#include "cj_stage.hpp"
#include "cj_match.hpp"

namespace cj {

#define CJ_LANES(lane) for (uint32_t lane = lane_id(); lane < 64u; lane += 64u)

__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) { return uni(*p); }
__device__ __forceinline__ uint32_t lds_ld8(const uint8_t* p) { return uni((uint32_t)*p); }
__device__ __forceinline__ void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_xor(uint32_t* p, uint32_t v) { atomicXor(p, v); }
__device__ __forceinline__ void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ uint32_t in_ld8(const uint8_t* p) { return *p; }
__device__ __forceinline__ uint32_t in_ld32(const uint8_t* p) { return ld32u(p); }
__device__ __forceinline__ uint32_t out_ld8(const uint8_t* p) { return uni((uint32_t)*p); }
__device__ __forceinline__ uint32_t out_rd32(const uint8_t* p) { return ld32u(p); }
__device__ __forceinline__ void out_st8(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }
typedef uint32_t lane_u32_unaligned __attribute__((aligned(1)));
__device__ __forceinline__ void out_st32(uint8_t* p, uint32_t v) { *reinterpret_cast<lane_u32_unaligned*>(p) = v; }
__device__ __forceinline__ void slot_st8(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }

struct LaneBytes {
    uint32_t v;
    __device__ __forceinline__ void put(uint32_t k, uint32_t byte) { if (lane_id() == k) v = byte; }
    __device__ __forceinline__ void flush(uint8_t* dst, uint32_t n) { if (lane_id() < n) dst[lane_id()] = (uint8_t)v; }
};
struct LaneU32 { uint32_t v; __device__ __forceinline__ uint32_t& operator[](uint32_t) { return v; } };
struct LaneU64 { uint64_t v; __device__ __forceinline__ uint64_t& operator[](uint32_t) { return v; } };
__device__ __forceinline__ uint32_t lane_excl_add(LaneU32& x, LaneU32& before) {
    uint32_t total;
    before.v = wave_excl_add(x.v, total);
    return total;
}

}  // namespace cj
