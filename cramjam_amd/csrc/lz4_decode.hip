// lz4_decode.hip — LZ4 *block* decoder for gfx950, one wavefront per independent chunk.
//
// Replaces (on the GPU) what the reference reaches at /root/reference/src/lz4.rs:88,90,164,168:
// libcramjam::lz4::block::decompress_into -> lz4 crate -> LZ4_decompress_safe.  Accept/reject rules
// follow the liblz4 1.10.0 safe decoder (end-of-block parsing restrictions relative to the decode
// capacity, variable-length field limits); offset 0 is rejected (spec-invalid).
//
// Shape: the sequence grammar is parsed wave-uniformly on the scalar unit out of a 512-byte register
// window (v_readlane), the vector lanes only move bytes: literals HBM->HBM, matches from the
// chunk's own freshly written output (same-wave L1-coherent), byte per lane, 16 B/lane on long runs.
// The decoder itself is lz4_wave.hpp (lz4_wave_decode<false>: the text the host build runs too); here are its two kernels.
#include "cj_engine.hpp"
#include "lz4_lane_walk.hpp"
#include "snappy_records.hpp"
#include "lz4_wave.hpp"

namespace cj {

// route: nullptr = decode every chunk; else only chunks the parse stage flagged kRouteWave.
__global__ __launch_bounds__(kBlockThreads) void lz4_decode_kernel(BatchArgs a, const ParseMeta* route) {
    const uint32_t chunk = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (chunk >= a.n_chunks) return;
    if (route != nullptr && (route[chunk].in_skip & kRouteWave) == 0u) return;
    const uint8_t* in = a.in_base + a.in_off[chunk];
    uint64_t n64 = a.in_len[chunk];
    uint8_t* out = a.out_base + a.out_off[chunk];
    uint64_t cap64 = a.out_cap[chunk];
    int64_t status = 0;

    // (lz4_block_prologue's rules, lz4_lane_walk.hpp, written out: DESIGN.md §5.10a)
    if (a.flags & CJ_FLAG_LZ4_SIZE_PREFIX) {
        // lz4 crate decompress_to_buffer(src, None, buffer): u32-LE size prefix (reference src/lz4.rs:90,164)
        if (n64 < 4) { status = CJ_E_NO_PREFIX; }
        else {
            int32_t size = (int32_t)((uint32_t)in[0] | ((uint32_t)in[1] << 8) | ((uint32_t)in[2] << 16) | ((uint32_t)in[3] << 24));
            if (size < 0) status = CJ_E_NEG_PREFIX;
            else if ((uint32_t)size > 0x7E000000u) status = CJ_E_PREFIX_TOO_BIG;
            else if ((uint64_t)size > cap64) status = CJ_E_OUT_TOO_SMALL;
            else { in += 4; n64 -= 4; cap64 = (uint64_t)size; }
        }
    } else {
        // capacity is handed to liblz4 as an i32
        int32_t size = (int32_t)(uint32_t)cap64;
        if (cap64 > 0xFFFFFFFFull || size < 0) status = CJ_E_NEG_PREFIX;
        else if ((uint32_t)size > 0x7E000000u) status = CJ_E_PREFIX_TOO_BIG;
    }
    if (status == 0 && n64 > 0x7FFFFFF0ull) status = CJ_E_CORRUPT;
    if (status != 0) { if (lane_id() == 0) a.result[chunk] = status; return; }

    const int64_t r = lz4_wave_decode<false>(in, (uint32_t)n64, out, (uint32_t)cap64, nullptr, 0u);
    if (lane_id() == 0) a.result[chunk] = r;
}

// ---------------------------------------------------------------------------------------------------
// LZ4 FRAMES with LINKED blocks (frame.hip, frame_batch.hip): block k may copy from the previous 64 KiB of output, so the
// blocks of a frame form a chain.  One wavefront per frame walks them in order and decodes straight into the frame's
// contiguous output; stored blocks are copied.  word[k] = block size | bit 31 (stored).  result[k] = decoded size or
// CJ_E_CORRUPT; the walk stops at the first bad block.  (Slow by construction — one wave, one dependency chain; frames
// with independent blocks take the batch path instead.)  jobs == nullptr: the one frame `one` (grid of one wavefront).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void lz4_frame_chain_kernel(const uint8_t* in, const uint64_t* blk_off, const uint32_t* word,
                                                             uint8_t* out_base, int64_t* result, const ChainJob* jobs, ChainJob one) {
    const ChainJob j = jobs != nullptr ? jobs[blockIdx.x] : one;
    const uint32_t nblk = uni(j.nblk), block_max = uni(j.block_max);
    uint8_t* out = out_base + j.out_off;
    const uint64_t out_cap = j.out_cap;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < nblk; i++) {
        const uint64_t k = j.blk0 + i;
        const uint32_t wd = uni(word[k]);
        const uint32_t sz = wd & 0x7FFFFFFFu;
        const uint8_t* src = in + blk_off[k];
        const uint64_t room = out_cap - pos;
        int64_t r;
        if (wd & 0x80000000u) {
            if (sz > room) r = CJ_E_CORRUPT;
            else { wave_copy(out + pos, src, sz); r = (int64_t)sz; }
        } else {
            const uint32_t cap = room < block_max ? (uint32_t)room : block_max;
            r = lz4_wave_decode<false>(src, sz, out + pos, cap, nullptr, pos < 65536u ? (uint32_t)pos : 65536u);
        }
        if (lane_id() == 0) result[k] = r;
        if (r < 0) {
            for (uint32_t m = i + 1 + lane_id(); m < nblk; m += 64u) result[j.blk0 + m] = CJ_E_CORRUPT;
            return;
        }
        pos += (uint64_t)r;
        wave_order();
    }
}

void launch_lz4_frame_chain(const uint8_t* in, const uint64_t* blk_off, const uint32_t* word, uint32_t nblk, uint8_t* out,
                            uint64_t out_cap, uint32_t block_max, int64_t* result, hipStream_t s) {
    if (nblk == 0) return;
    const ChainJob one = { 0, 0, out_cap, nblk, block_max };
    hipLaunchKernelGGL(lz4_frame_chain_kernel, dim3(1), dim3(64), 0, s, in, blk_off, word, out, result, (const ChainJob*)nullptr, one);
}

void launch_lz4_frame_chains(const uint8_t* in, const uint64_t* blk_off, const uint32_t* word, uint8_t* out_base, int64_t* result,
                             const ChainJob* jobs, uint32_t n_jobs, hipStream_t s) {
    if (n_jobs == 0) return;
    hipLaunchKernelGGL(lz4_frame_chain_kernel, dim3(n_jobs), dim3(64), 0, s, in, blk_off, word, out_base, result, jobs, ChainJob{});
}

void launch_lz4_decode(const BatchArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return;
    hipLaunchKernelGGL(lz4_decode_kernel, wave_grid(a.n_chunks), dim3(kBlockThreads), 0, s, a, (const ParseMeta*)nullptr);
}

void launch_lz4_decode_routed(const BatchArgs& a, const void* meta, hipStream_t s) {
    if (a.n_chunks == 0) return;
    hipLaunchKernelGGL(lz4_decode_kernel, wave_grid(a.n_chunks), dim3(kBlockThreads), 0, s, a, (const ParseMeta*)meta);
}


}  // namespace cj
