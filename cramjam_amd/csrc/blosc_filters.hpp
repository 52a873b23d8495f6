// blosc_filters.hpp — the block list of the Blosc filter kernels (blosc_filters.hip) and their tiling.  Not part of the C-ABI.
#pragma once
#include "cj_stage.hpp"
#include "blosc_grammar.hpp"

namespace cj {

// one block of one chunk: `bytes` bytes from src to dst (device addresses), mode = blosc_block_mode of the chunk's flags
struct BloscBlockRow {
    uint64_t src, dst;
    uint32_t bytes, typesize, mode, chunk;
};

constexpr uint32_t kBloscTileBytes = 16384;
// elements per tile: the largest power of two with E x typesize <= 16 KiB, 64 .. 4096
CJ_HD inline uint32_t blosc_tile_elems(uint32_t typesize) {
    uint32_t e = 4096;
    while (e > 64 && e * typesize > kBloscTileBytes) e >>= 1;
    return e;
}
// tiles that cover a block of `bytes` bytes in any mode (copy: 16 KiB each)
CJ_HD inline uint32_t blosc_tiles(uint32_t typesize, uint32_t bytes) {
    const uint32_t e = blosc_tile_elems(typesize);
    const uint32_t a = (bytes / typesize + e - 1) / e, b = (bytes + kBloscTileBytes - 1) / kBloscTileBytes;
    return a > b ? (a ? a : 1u) : (b ? b : 1u);
}

// forward: filter (compress side), else unfilter.  tiles_max: at least blosc_tiles of every row.  gate: per-chunk results, rows of a
// chunk with a negative one are skipped (nullptr: none are).  Enqueue only.
void launch_blosc_filter(const BloscBlockRow* rows, size_t n_rows, uint32_t tiles_max, bool forward, const int64_t* gate, hipStream_t s);

// blosclz_decode.hip: one wavefront per row of a decodes a BloscLZ stream of in_len bytes into exactly out_cap bytes: result = out_cap or
// CJ_E_CORRUPT; a row with out_cap == 0 is skipped (result 0).  Nothing is written beyond out_off + out_cap.  Enqueue only.
void launch_blosclz_decode(const BatchArgs& a, hipStream_t s);

// The streams of Zlib / Zstd chunks (CJ_BLOSC_FLAG_READ_ZLIB / _ZSTD), one wavefront per row of a, by the decoders of the plain batches:
// result = the decoded length (good iff it is out_cap) or a CJ_E_DEFLATE_* / CJ_E_ZSTD_* code.  A row of a stored stream (in_len and
// out_cap 0) reads and writes nothing; its result (0 or a code) is not looked at.  Both decoders check every store against
// out_off + out_cap (the wave-decoder contract).  0 or CJ_E_*; enqueue only.
// deflate.hip: deflate_launch for CJ_DEFLATE_ZLIB, not in size mode
int launch_zlib_decode(const BatchArgs& a, hipStream_t s);
// ... for CJ_DEFLATE_GZIP: the members of BGZF streams (bgzf_batch.hip) and the GZIP pages of Parquet chunks (parquet_batch.hip), one row each
int launch_gzip_decode(const BatchArgs& a, hipStream_t s);
// ... for CJ_DEFLATE_RAW: the compressed chunks of ORC streams with ZLIB (orc_batch.hip), one row each
int launch_deflate_raw_decode(const BatchArgs& a, hipStream_t s);
// zstd.hip: the decode of cj_zstd_batch_device — its own cj::ScratchTurn on e->zstd_slots, slices by the literal-slot budget
int launch_zstd_decode(::cj_engine* e, const BatchArgs& a, hipStream_t s);

// The size queries of the plain batches over rows of a container (orc_batch.hip: ORC states no chunk's decoded length): result[i] = the
// decoded length or the code cj_*_batch_sizes_device gives; a row with in_len 0 reads nothing.  No scratch; 0 or CJ_E_*; enqueue only.
// deflate.hip: deflate_launch for CJ_DEFLATE_RAW in size mode
int launch_deflate_raw_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s);
// batch_sizes.hip: codec = CJ_CODEC_LZ4_BLOCK (raw blocks: the size walk) or CJ_CODEC_SNAPPY_RAW (the header's length)
int launch_block_sizes(int codec, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s);
// zstd.hip: the decoder without stores
int launch_zstd_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s);

}  // namespace cj
