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

}  // namespace cj
