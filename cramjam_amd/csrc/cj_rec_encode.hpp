// cj_rec_encode.hpp — what the encoders that code sequence records share on the device (deflate_encode.hip, zstd_encode.hip; DESIGN.md
// §5.13, §5.15): the record's load and the matcher's format.  Stage 1 of both is enc2::Walk<RecFmt<kMaxDist>, 2> (cj_enc2.hpp: the
// matcher of the LZ4 and Snappy encoders), which leaves fixed-size sequence records in the workgroup's scratch slot; stage 2 is the
// format's entropy stage (deflate_enc_wave.hpp, zstd_enc_wave.hpp) over rec_ld.  Not part of the C-ABI.
#pragma once
#include "wave_lanes.hpp"
#include "cj_enc2.hpp"

namespace cj {

struct DfeRec;
__device__ __forceinline__ DfeRec rec_ld(const DfeRec* slot, uint32_t i);

}  // namespace cj

#include "deflate_enc_wave.hpp"      // (DfeRec, kDfePiece and kDfeSlotRecs stay with the entropy stage: the host builds compile its text)

namespace cj {

__device__ __forceinline__ DfeRec rec_ld(const DfeRec* slot, uint32_t i) {
    const uint4 v = *reinterpret_cast<const uint4*>(slot + i);
    return DfeRec{v.x, v.y, v.z, v.w};
}

// The matcher's format: a sequence is one record in the scratch slot (`out`), counted in records.  kMaxDist: DEFLATE's 32 768;
// Zstandard's 65 535 is the lap of the matcher's 16-bit table — a match starts at most 8 bytes before a piece's end (last_start), so
// the largest distance a 64 KiB piece holds is 65 528: that limit is never the one that binds, and offset code 16 (Offset_Value >=
// 65 536) never occurs
template <uint32_t kMaxDist_>
struct RecFmt {
    static constexpr uint32_t kMaxDist = kMaxDist_;
    static constexpr bool kStreamLiterals = false;
    static __device__ __forceinline__ uint32_t last_start(uint32_t n) { return n - 8u; }      // Snappy's: the position lanes read 8 bytes at a time
    static __device__ __forceinline__ uint32_t limit(uint32_t n) { return n; }
    static __device__ __forceinline__ uint32_t seq_size(uint32_t, uint32_t, uint32_t) { return 1u; }
    static __device__ __forceinline__ void put(enc2::gptr out, uint32_t o, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen) {
        if (o + 1u < kDfeSlotRecs) enc2::s128(out, 16u * o, make_uint4(lit0, lit, off, mlen));      // (the last record is the final literals')
    }
    static __device__ __forceinline__ uint32_t emit_lane(enc2::gcptr, enc2::gptr out, uint32_t o, uint32_t lit0, uint32_t lit, uint32_t code, uint32_t off) {
        put(out, o, lit0, lit, off, code + 4u);
        return 0u;
    }
    static __device__ __forceinline__ uint32_t emit_wave(enc2::gcptr, enc2::gptr out, uint32_t op, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen) {
        if (lane_id() == 0u) put(out, op, lit0, lit, off, mlen);
        return op + 1u;
    }
};

constexpr uint32_t kRecBytes = (kDfeSlotRecs * 16u + 255u) & ~255u;      // the records of a scratch slot
constexpr int kRecEncThreads = 128;                                       // two wavefronts a stream

}  // namespace cj
