// blosc_grammar.hpp — the grammar of a Blosc1-format chunk (c-blosc 1.x, format version 2: 16-byte header) whose compressor format
// is LZ4 (or, where the caller's flags ask for it, BloscLZ, Zlib or Zstd), for the host (one chunk per call, cj_blosc_chunk_info) and the device (blosc_batch.hip: one lane per chunk).  The walk checks
// the header and the block table, reports every stream to a visitor and returns 0 or the first error.  Format rules only: no staging,
// no decoding, no filters.  Every read stays inside [chunk, chunk + in_len).  Not part of the C-ABI.
//
//   header   version = 2 | versionlz | flags | typesize | nbytes u32 | blocksize u32 | cbytes u32            (little endian)
//   flags    0x01 byte shuffle, 0x02 memcpyed, 0x04 bitshuffle, 0x10 blocks are not split, bits 5..7 compressor format (1 = LZ4,
//            0 = BloscLZ, 3 = Zlib, 4 = Zstd: each read only with its CJ_BLOSC_FLAG_READ_* in the caller's flags; 2 = Snappy: never)
//   memcpyed nbytes raw bytes behind the header
//   else     nblocks = ceil(nbytes / blocksize) u32 bstarts (from the chunk's start); block = nsplits streams of i32 cbytes + payload;
//            nsplits = typesize iff 0x10 is clear and the block is not the leftover block (nbytes % blocksize != 0: the last one),
//            else 1; a stream decodes to block_bytes / nsplits bytes: stored raw when its cbytes says exactly that, else one LZ4 block
//            (one BloscLZ stream: blosclz_decode.hip; one zlib stream: deflate.hip; one ZSTD_decompress input: zstd.hip)
// The 32-byte header of C-Blosc2 (format version > 2) is refused, not guessed at: DESIGN.md §5.10.
#pragma once
#include "frame_grammar.hpp"

namespace cj {

constexpr uint32_t kBloscHeader = 16;
constexpr uint32_t kBloscMaxBytes = 0x7FFFFFFFu - 16u;     // BLOSC_MAX_BUFFERSIZE
constexpr uint32_t kBloscShuffle = 1, kBloscMemcpyed = 2, kBloscBitshuffle = 4, kBloscReserved = 8, kBloscNoSplit = 16;
constexpr uint32_t kBloscFormatBlosclz = 0, kBloscFormatLz4 = 1, kBloscFormatSnappy = 2, kBloscFormatZlib = 3, kBloscFormatZstd = 4;

struct BloscHeader {
    uint32_t version, versionlz, flags, typesize, nbytes, blocksize, cbytes;
    uint32_t nblocks;             // 0 for a memcpyed or empty chunk
    uint32_t format;              // compressor format of the streams (kBloscFormat*); kBloscFormatLz4 where the chunk has none
};

struct BloscStream {
    uint32_t src_off, src_len;    // payload in the chunk
    uint32_t dst_off, dst_len;    // decoded bytes in the (still filtered) chunk image
    uint32_t block;
    bool stored;
};

// what the filter stage does with a block (blosc_filters.hip); the forward direction is the same number
enum BloscFilterMode : uint32_t { kBloscCopy = 0, kBloscByte = 1, kBloscBit = 2 };

// the filter of a block of `bytes` bytes by c-blosc's rules: byte shuffle only for typesize > 1; bitshuffle only for a block of at
// least one element whose element count is a multiple of 8 (any other block is left as it is)
CJ_HD inline uint32_t blosc_block_mode(uint32_t flags, uint32_t typesize, uint32_t bytes) {
    if ((flags & kBloscShuffle) && typesize > 1) return kBloscByte;
    if ((flags & kBloscBitshuffle) && bytes >= typesize && (bytes / typesize) % 8u == 0) return kBloscBit;
    return kBloscCopy;
}

// the 8 x 8 bit transposition of bitshuffle: byte k of x = one byte of element k -> byte p of the result = bit plane p (bit k of it =
// bit p of element k's byte).  Three masked shift-xor steps; its own inverse.
CJ_HD inline uint64_t blosc_tr8(uint64_t x) {
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}

// header checks alone: 0, CJ_E_BLOSC_HEADER or CJ_E_BLOSC_UNSUPPORTED.  The ORDER of the checks is relied on outside this file:
// cramjam_amd/blosc2.py _info_nbytes sizes the output of a BloscLZ, Zlib or Zstd chunk from cj_blosc_chunk_info (which passes no flags) by taking
// back exactly the compressor-format refusal below, the last check before the block table's — keep the two together.  read_flags: the caller's flags word (CJ_BLOSC_FLAG_*; 0 = the
// default reading: LZ4 streams only)
CJ_HD inline int64_t blosc_header(const uint8_t* in, size_t in_len, BloscHeader& h, uint32_t read_flags = 0) {
    h = BloscHeader{};
    h.format = kBloscFormatLz4;
    if (in_len < kBloscHeader) return CJ_E_BLOSC_HEADER;
    h.version = in[0]; h.versionlz = in[1]; h.flags = in[2]; h.typesize = in[3];
    h.nbytes = fg_rd32(in + 4); h.blocksize = fg_rd32(in + 8); h.cbytes = fg_rd32(in + 12);
    if (h.version != 2) return CJ_E_BLOSC_UNSUPPORTED;                    // 1: pre-1.0 Blosc; 3 and up: C-Blosc2's extended header
    if ((h.flags & kBloscReserved) || (h.flags & (kBloscShuffle | kBloscBitshuffle)) == (kBloscShuffle | kBloscBitshuffle)) return CJ_E_BLOSC_HEADER;
    if (h.typesize == 0) return CJ_E_BLOSC_HEADER;
    if (h.cbytes < kBloscHeader || h.cbytes > in_len) return CJ_E_BLOSC_HEADER;
    if (h.nbytes > kBloscMaxBytes) return CJ_E_BLOSC_HEADER;
    if (h.nbytes == 0) return 0;                                           // (an empty chunk: nothing else is looked at)
    if (h.blocksize == 0 || h.blocksize > h.nbytes) return CJ_E_BLOSC_HEADER;
    if (h.flags & kBloscMemcpyed) return h.cbytes == h.nbytes + kBloscHeader ? 0 : (int64_t)CJ_E_BLOSC_HEADER;
    const uint32_t fmt = h.flags >> 5;
    const bool opted = (fmt == kBloscFormatBlosclz && (read_flags & CJ_BLOSC_FLAG_READ_BLOSCLZ)) || (fmt == kBloscFormatZlib && (read_flags & CJ_BLOSC_FLAG_READ_ZLIB)) ||
                       (fmt == kBloscFormatZstd && (read_flags & CJ_BLOSC_FLAG_READ_ZSTD));
    if ((fmt != kBloscFormatLz4 && !opted) || h.versionlz != 1) return CJ_E_BLOSC_UNSUPPORTED;     // BloscLZ 0, Snappy 2, Zlib 3, Zstd 4
    h.format = h.flags >> 5;
    const uint64_t nblocks = ((uint64_t)h.nbytes + h.blocksize - 1) / h.blocksize;
    if (kBloscHeader + 4 * nblocks > h.cbytes) return CJ_E_BLOSC_HEADER;
    h.nblocks = (uint32_t)nblocks;
    return 0;
}

// f(const BloscStream&) for every stream in block order.  Returns 0 or the first error.
template <class F>
CJ_HD inline int64_t blosc_walk(const uint8_t* in, size_t in_len, BloscHeader& h, F&& f, uint32_t read_flags = 0) {
    const int64_t err = blosc_header(in, in_len, h, read_flags);
    if (err != 0) return err;
    const uint32_t table_end = kBloscHeader + 4 * h.nblocks;
    const uint32_t leftover = h.nbytes % h.blocksize;
    // Block starts may come in any order (c-blosc's threads claim their places as they finish), so overlapping blocks cannot be told
    // from the table alone; but streams that do not overlap take 5 bytes each at least, and a chunk that claims more than cbytes / 5
    // of them is refused: what a hostile chunk can make a batch reserve stays proportional to its own size
    uint64_t budget = h.cbytes / 5u;
    for (uint32_t b = 0; b < h.nblocks; b++) {
        const bool last_short = leftover != 0 && b + 1 == h.nblocks;
        const uint32_t bytes = last_short ? leftover : h.blocksize;
        const uint32_t nsplits = (!(h.flags & kBloscNoSplit) && !last_short) ? h.typesize : 1u;
        if (bytes % nsplits != 0 || nsplits > budget) return CJ_E_BLOSC_HEADER;
        budget -= nsplits;
        const uint32_t each = bytes / nsplits;
        uint64_t pos = fg_rd32(in + kBloscHeader + 4 * b);
        if (pos < table_end) return CJ_E_BLOSC_HEADER;
        for (uint32_t k = 0; k < nsplits; k++) {
            if (pos + 4 > h.cbytes) return CJ_E_BLOSC_HEADER;
            const int32_t cb = (int32_t)fg_rd32(in + pos);
            if (cb <= 0 || pos + 4 + (uint64_t)cb > h.cbytes) return CJ_E_BLOSC_HEADER;
            BloscStream s;
            s.src_off = (uint32_t)pos + 4; s.src_len = (uint32_t)cb;
            s.dst_off = b * h.blocksize + k * each; s.dst_len = each;
            s.block = b; s.stored = (uint32_t)cb == each;
            f(s);
            pos += 4 + (uint64_t)cb;
        }
    }
    return 0;
}

// ---- the writer's side (blosc_batch.hip compress) ------------------------------------------------------------------------------
// Block size of this library's chunks: 64 KiB x typesize split into typesize streams when typesize <= 16 and a stream gets at least
// 128 bytes, else 64 KiB unsplit (flag 0x10).  Every stream is then at most 64 KiB: one chunk of the batch encoders.  `want`
// (0 = default) is a caller's block size; one above the default is cut to it, and a chunk whose leftover block would exceed 64 KiB is
// written unsplit, so that the bound holds.
struct BloscLayout { uint32_t blocksize, nblocks; bool split; };
CJ_HD inline BloscLayout blosc_layout(uint32_t nbytes, uint32_t typesize, uint32_t want) {
    BloscLayout l;
    l.split = typesize > 1 && typesize <= 16;
    const uint32_t def = 65536u * (l.split ? typesize : 1u);
    uint32_t bs = (want && want <= def) ? want : def;
    if (bs > nbytes) bs = nbytes;
    if (l.split) bs -= bs % typesize;                      // whole elements (what is left of the chunk becomes the leftover block)
    if (l.split && bs / typesize < 128u) { l.split = false; bs = bs ? bs : nbytes; if (bs > 65536u) bs = 65536u; }
    if (l.split && nbytes % bs > 65536u) { l.split = false; bs = 65536u; }      // (the leftover block is one stream: it keeps the bound too)
    l.blocksize = bs;
    l.nblocks = nbytes ? (uint32_t)(((uint64_t)nbytes + bs - 1) / bs) : 0u;
    return l;
}

}  // namespace cj
