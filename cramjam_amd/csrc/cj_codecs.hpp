// cj_codecs.hpp — the inner codecs of the container batches (blosc_batch.hip, bgzf_batch.hip, orc_batch.hip, parquet_batch.hip; DESIGN.md
// §5.16a): what a container entry can be, and the ONE call of "the codec's plain batch" over the entry rows, in both directions and
// for the size query.  The containers' grammars (orc_grammar.hpp, parquet_grammar.hpp) map their kinds to an Inner and build for the
// host too, so the first part needs the C ABI's header alone; the launchers and the dispatch are the device build's.  Not part of the C ABI.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/cramjam_hip.h"

namespace cj {

// the streams a container entry can be
enum Inner { kInLz4Raw, kInSnappyRaw, kInDeflateRaw, kInZlib, kInGzip, kInZstd, kInBloscLz };
constexpr bool inner_is_block(Inner c) { return c == kInLz4Raw || c == kInSnappyRaw; }
constexpr bool inner_is_deflate(Inner c) { return c == kInDeflateRaw || c == kInZlib || c == kInGzip; }
constexpr cj_codec inner_block_codec(Inner c) { return c == kInLz4Raw ? CJ_CODEC_LZ4_BLOCK : CJ_CODEC_SNAPPY_RAW; }
constexpr int inner_wrap(Inner c) { return c == kInDeflateRaw ? CJ_DEFLATE_RAW : c == kInZlib ? CJ_DEFLATE_ZLIB : CJ_DEFLATE_GZIP; }

// The engine's size class for LZ4 / Snappy rows none of which decodes to more than `largest` bytes, as far as the host knows: a hint
// that a row may break (the decoders route such a row themselves)
constexpr uint32_t size_class_flags(uint64_t largest) {
    return largest <= 16384u ? CJ_FLAG_CHUNKS_LE_16K : largest <= 32768u ? CJ_FLAG_CHUNKS_LE_32K : largest > 65536u ? CJ_FLAG_BIG_CHUNKS : 0u;
}
static_assert(size_class_flags(16384) == CJ_FLAG_CHUNKS_LE_16K && size_class_flags(16385) == CJ_FLAG_CHUNKS_LE_32K, "the 16 KiB class ends at 16384");
static_assert(size_class_flags(32768) == CJ_FLAG_CHUNKS_LE_32K && size_class_flags(32769) == 0u, "the 32 KiB class ends at 32768");
static_assert(size_class_flags(65536) == 0u && size_class_flags(65537) == CJ_FLAG_BIG_CHUNKS, "big chunks begin at 65537");

// what the codec's encoder may write for n bytes (0: it has none)
inline size_t inner_bound(Inner c, size_t n) {
    return inner_is_deflate(c) ? cj_deflate_compress_bound(n, (cj_deflate_wrap)inner_wrap(c)) : c == kInSnappyRaw ? cj_snappy_raw_max_compress_len(n)
         : c == kInLz4Raw ? cj_lz4_block_compress_bound(n, 0) : c == kInZstd ? cj_zstd_compress_bound(n, 0) : 0;
}
// the codec's "corrupt", for a decode that ended short of its row's capacity without a code of its own
constexpr int64_t inner_short_code(Inner c) {
    return inner_is_deflate(c) ? CJ_E_DEFLATE_CORRUPT : c == kInSnappyRaw ? CJ_E_SNAPPY_CORRUPT : c == kInZstd ? CJ_E_ZSTD_CORRUPT : CJ_E_CORRUPT;
}

}  // namespace cj

#if defined(__HIPCC__)
#include "cj_engine.hpp"

namespace cj {

// ---- the per-codec launchers, one wavefront (BloscLZ, DEFLATE, Zstandard decode) or workgroup (the encoders) per row; LZ4 and Snappy
// blocks are cj::launch (cj_engine.hpp).  A decoder's result is the decoded length (good iff it is out_cap) or its CJ_E_* code, and every
// store is checked against out_off + out_cap (the wave-decoder contract); a row with in_len = out_cap = 0 (the
// stored-stream convention) reads and writes nothing, its result is not looked at.  0 or CJ_E_*; enqueue only.
// deflate.hip: what cj_deflate_batch_device / _sizes_device do behind their checks.  size: the size query — the output rows are not read
int launch_deflate(int wrap, bool size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                   const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s);
// zstd.hip: the decode of cj_zstd_batch_device — its own turn (slot_slices) on e->zstd_slots, slices by the literal-slot budget —, and
// the decoder without stores, which uses no scratch
int launch_zstd_decode(::cj_engine* e, const BatchArgs& a, hipStream_t s);
int launch_zstd_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s);
// blosclz_decode.hip: exactly out_cap bytes or CJ_E_CORRUPT; a row with out_cap == 0 is skipped (result 0)
void launch_blosclz_decode(const BatchArgs& a, hipStream_t s);
// batch_sizes.hip: codec = CJ_CODEC_LZ4_BLOCK (raw blocks: the size walk) or CJ_CODEC_SNAPPY_RAW (the header's length); a row with
// in_len 0 reads nothing.  No scratch
int launch_block_sizes(int codec, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s);
// deflate_encode.hip, zstd_encode.hip: what the public compress entries of either file do behind their checks — one stream / frame per row, their own turn (slot_slices) on e->deflate_slots / e->zstd_enc_slots, slices by the slot budget
int deflate_compress_device(::cj_engine* e, int wrap, const BatchArgs& b, hipStream_t s);
int zstd_compress_device(::cj_engine* e, uint32_t flags, const BatchArgs& b, hipStream_t s);

// ---- the dispatch.  A container calls these inside its e->fb turn (lock order: cj_engine.hpp); an empty range launches nothing.
// One codec launch over the rows, straight to out_base.  `largest` bounds every row's capacity (LZ4 and Snappy's size class)
inline int inner_decode(::cj_engine* e, Inner c, uint64_t largest, const uint8_t* in_base, uint8_t* out_base, const BatchRows& r, hipStream_t s) {
    if (r.n == 0) return 0;
    if (inner_is_deflate(c)) return launch_deflate(inner_wrap(c), /*size=*/false, r.n, in_base, r.in_off, r.in_len, out_base, r.out_off, r.out_cap, r.result, s);
    BatchArgs a;
    fill_args(a, inner_is_block(c) ? size_class_flags(largest) : 0u, in_base, out_base, r);
    if (inner_is_block(c)) return launch(e, inner_block_codec(c), CJ_OP_DECOMPRESS, a, s);
    if (c == kInZstd) return launch_zstd_decode(e, a, s);
    launch_blosclz_decode(a, s);
    return 0;
}

// the codec's size query over the rows: its answers into their result row (BloscLZ states no length: none)
inline int inner_sizes(Inner c, const uint8_t* in_base, const BatchRows& r, hipStream_t s) {
    if (r.n == 0) return 0;
    if (inner_is_deflate(c)) return launch_deflate(inner_wrap(c), /*size=*/true, r.n, in_base, r.in_off, r.in_len, nullptr, nullptr, nullptr, r.result, s);
    if (inner_is_block(c)) return launch_block_sizes(inner_block_codec(c), r.n, in_base, r.in_off, r.in_len, r.result, s);
    return c == kInZstd ? launch_zstd_sizes(r.n, in_base, r.in_off, r.in_len, r.result, s) : CJ_E_BAD_ARG;
}

// the first cnt rows through the codec's encoder (BloscLZ has none)
inline int inner_encode(::cj_engine* e, Inner c, const uint8_t* in_base, uint8_t* out_base, const BatchRows& r, uint32_t cnt, hipStream_t s) {
    if (cnt == 0) return 0;
    BatchArgs a;
    fill_args(a, 0, cnt, in_base, r.in_off, r.in_len, out_base, r.out_off, r.out_cap, r.result);
    if (inner_is_deflate(c)) return deflate_compress_device(e, inner_wrap(c), a, s);
    if (inner_is_block(c)) return launch(e, inner_block_codec(c), CJ_OP_COMPRESS, a, s);
    return c == kInZstd ? zstd_compress_device(e, 0u, a, s) : CJ_E_BAD_ARG;
}

// ---- the entry rows of a container whose entries are coded or copied: the codec's batch and the copy_segments rows of the entries that
// are copied (a copied entry's codec row is the stored-stream convention's).  FbRows (cj_stage.hpp) begins the same way and stays on its
// own: the frame batches are a single-turn protocol below this header that names no Inner.
struct CopyRows {
    BatchRows b;
    uint64_t *cp_src, *cp_dst, *cp_len;
};
constexpr size_t kBatchRowWords = 5, kCopyRowWords = kBatchRowWords + 3;      // u64 rows per entry of batch_rows / copy_rows
inline CopyRows copy_rows(uint64_t* base, size_t n) {
    CopyRows r;
    r.b = batch_rows(base, n);
    r.cp_src = r.b.end; r.cp_dst = r.b.end + n; r.cp_len = r.b.end + 2 * n;
    return r;
}

}  // namespace cj
#endif
