// frame_grammar.hpp — the grammar of the two framed formats, for the host (frame.hip: one stream per call) and the device
// (frame_batch.hip: one lane per stream).  A walk reports every block it finds to a visitor and returns the first
// header-level error; what it meets after the first block is a LATE error (the blocks before it are intact and a streaming
// decoder would have written them).  Format rules only: no staging, no checksums of the payload.  Not part of the C-ABI.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/cramjam_hip.h"

#if defined(__HIPCC__)
#define CJ_HD __host__ __device__
#else
#define CJ_HD
#endif

namespace cj {

CJ_HD inline uint32_t fg_rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
CJ_HD inline uint32_t fg_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 of a short byte string (the LZ4 frame descriptor: at most 14 bytes), seed 0
CJ_HD inline uint32_t xxh32_short(const uint8_t* p, uint32_t n) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    uint32_t h = P5 + n, i = 0;
    for (; i + 4 <= n; i += 4) h = fg_rotl(h + fg_rd32(p + i) * P3, 17) * P4;
    for (; i < n; i++) h = fg_rotl(h + (uint32_t)p[i] * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// the varint in front of a Snappy raw block (cj_snappy_raw_decompress_len)
CJ_HD inline int64_t snappy_varint_len(const uint8_t* in, size_t n) {
    if (n == 0) return 0;
    uint64_t v = 0;
    unsigned shift = 0;
    for (size_t i = 0; i < n && i < 10; i++) {
        const uint8_t b = in[i];
        if (b < 0x80) {
            if (i == 9 && b > 1) return CJ_E_SNAPPY_HEADER;
            v |= (uint64_t)b << shift;
            return v > 0xFFFFFFFFull ? (int64_t)CJ_E_SNAPPY_TOO_BIG : (int64_t)v;
        }
        v |= (uint64_t)(b & 0x7f) << shift;
        shift += 7;
    }
    return CJ_E_SNAPPY_HEADER;
}

// ---- Snappy framing format (snap read::FrameDecoder::read) ---------------------------------------------------------------
constexpr uint32_t kSnapPiece = 65536;          // snap MAX_BLOCK_SIZE
constexpr uint32_t kSnapMaxChunk = 76490;       // snap MAX_COMPRESS_BLOCK_SIZE = max_compress_len(65536)

struct SnapPiece {
    uint64_t src_off;     // payload offset in the framed stream
    uint64_t dst_off;     // offset of the decoded piece in the output
    uint32_t src_len, dst_len, crc;
    bool stored;
};

// Walks the chunk grammar; visit(const SnapPiece&) for every data chunk.  Returns 0 or the first header-level error (the pieces
// before it were visited: snap would have decoded those first, so their errors take precedence); *total = decoded bytes listed.
template <class V>
CJ_HD int64_t snappy_frame_walk(const uint8_t* in, size_t n, V&& visit, uint64_t* total) {
    const uint8_t ident[6] = { 's', 'N', 'a', 'P', 'p', 'Y' };
    size_t pos = 0;
    uint64_t op = 0;
    bool have_ident = false;
    int64_t err = 0;
    while (pos < n) {
        if (n - pos < 4) { err = CJ_E_FRAME_EOF; break; }
        const uint8_t ty = in[pos];
        if (!have_ident) {
            if (ty != 0xff) { err = CJ_E_SNAPPY_STREAM_HEADER; break; }
            have_ident = true;
        }
        const size_t len = (size_t)in[pos + 1] | ((size_t)in[pos + 2] << 8) | ((size_t)in[pos + 3] << 16);
        if (len > kSnapMaxChunk) { err = CJ_E_SNAPPY_CHUNK_LEN; break; }
        pos += 4;
        if (ty >= 0x02 && ty <= 0x7f) { err = CJ_E_SNAPPY_CHUNK_TYPE; break; }
        if (ty >= 0x80 && ty <= 0xfe) {                 // reserved skippable, padding
            if (n - pos < len) { err = CJ_E_FRAME_EOF; break; }
            pos += len;
            continue;
        }
        if (ty == 0xff) {
            if (len != 6) { err = CJ_E_SNAPPY_CHUNK_LEN; break; }
            if (n - pos < 6) { err = CJ_E_FRAME_EOF; break; }
            bool same = true;
            for (int k = 0; k < 6; k++) same = same && in[pos + k] == ident[k];
            if (!same) { err = CJ_E_SNAPPY_STREAM_HEADER; break; }
            pos += 6;
            continue;
        }
        if (len < 4) { err = CJ_E_SNAPPY_CHUNK_LEN; break; }
        if (n - pos < 4) { err = CJ_E_FRAME_EOF; break; }
        SnapPiece p;
        p.crc = fg_rd32(in + pos);
        pos += 4;
        const size_t sn = len - 4;
        p.stored = ty == 0x01;
        if (p.stored && sn > kSnapPiece) { err = CJ_E_SNAPPY_CHUNK_LEN; break; }
        if (n - pos < sn) { err = CJ_E_FRAME_EOF; break; }
        uint64_t dn = sn;
        if (!p.stored) {
            const int64_t d = snappy_varint_len(in + pos, sn);   // empty block -> 0; the decoder then reports Empty
            if (d < 0) { err = d; break; }
            if ((uint64_t)d > kSnapPiece) { err = CJ_E_SNAPPY_CHUNK_LEN; break; }
            dn = (uint64_t)d;
        }
        p.src_off = pos; p.src_len = (uint32_t)sn; p.dst_off = op; p.dst_len = (uint32_t)dn;
        visit(p);
        pos += sn;
        op += dn;
    }
    if (total) *total = op;
    return err;
}

// ---- LZ4 frame format (LZ4F_decompress's own checks; truncation = the lz4 crate's "Finish runned before read end ...") -------
struct Lz4Header {
    bool indep = true, bsum = false, csize = false, csum = false;
    bool skippable = false;
    bool complete = false;        // the EndMark was reached
    uint32_t block_max = 0;
    uint32_t content_sum = 0;
    uint64_t content_size = 0;
    int64_t late_err = 0;         // error met while walking the blocks (the blocks visited before it are intact)
};

// Header + block walk.  visit(src_off, word) for every block (word = size | bit 31 stored; its checksum, if the frame has block
// checksums, follows the payload); a visitor that returns false stops the walk with late_err = CJ_E_LZ4F_BLOCK_CHECKSUM (the
// host checks block sums while walking).  Returns 0 or the header-level error.
template <class V>
CJ_HD int64_t lz4_frame_walk(const uint8_t* in, size_t n, Lz4Header& f, V&& visit) {
    if (n >= 8 && (fg_rd32(in) & 0xFFFFFFF0u) == 0x184D2A50u) {
        f.skippable = true;
        return n - 8 < fg_rd32(in + 4) ? (int64_t)CJ_E_LZ4F_INCOMPLETE : 0;
    }
    if (n < 7) return CJ_E_LZ4F_INCOMPLETE;
    if (fg_rd32(in) != 0x184D2204u) return CJ_E_LZ4F_FRAME_TYPE;
    const uint8_t flg = in[4], bd = in[5];
    if ((flg >> 6) != 1 || (flg & 0x02)) return CJ_E_LZ4F_HEADER;
    if ((bd & 0x8F) != 0) return CJ_E_LZ4F_HEADER;
    f.indep = (flg >> 5) & 1; f.bsum = (flg >> 4) & 1; f.csize = (flg >> 3) & 1; f.csum = (flg >> 2) & 1;
    const bool dictid = flg & 1;
    const uint32_t code = (bd >> 4) & 7;
    if (code < 4) return CJ_E_LZ4F_BLOCK_SIZE;
    f.block_max = 1u << (8 + 2 * code);
    const size_t hl = 6 + (f.csize ? 8 : 0) + (dictid ? 4 : 0);
    if (n < hl + 1) return CJ_E_LZ4F_INCOMPLETE;
    if (f.csize) f.content_size = (uint64_t)fg_rd32(in + 6) | ((uint64_t)fg_rd32(in + 10) << 32);
    if (in[hl] != (uint8_t)(xxh32_short(in + 4, (uint32_t)(hl - 4)) >> 8)) return CJ_E_LZ4F_HEADER;
    size_t pos = hl + 1;
    for (;;) {
        if (n - pos < 4) { f.late_err = CJ_E_LZ4F_INCOMPLETE; return 0; }
        const uint32_t w = fg_rd32(in + pos);
        pos += 4;
        if (w == 0) break;
        const size_t sz = w & 0x7FFFFFFFu;
        if (sz > f.block_max) { f.late_err = CJ_E_LZ4F_BLOCK_SIZE; return 0; }
        if (n - pos < sz + (f.bsum ? 4u : 0u)) { f.late_err = CJ_E_LZ4F_INCOMPLETE; return 0; }
        if (!visit((uint64_t)pos, w)) { f.late_err = CJ_E_LZ4F_BLOCK_CHECKSUM; return 0; }
        pos += sz + (f.bsum ? 4 : 0);
    }
    f.complete = true;
    if (f.csum) {
        if (n - pos < 4) { f.late_err = CJ_E_LZ4F_INCOMPLETE; return 0; }
        f.content_sum = fg_rd32(in + pos);
    }
    return 0;
}

// Scratch for one LZ4 block: a stored block its size, a compressed block of c bytes min(block_max, 255 c + 64) — what it can decode to
// at most (cj_lz4_frame_decompress_bound's rule: every sequence yields less than 255 bytes per input byte).  The block is decoded with
// that capacity instead of block_max: every capacity test of the safe decoder (room for a sequence's literals + 12, for a match + 5)
// then still passes wherever it passes with block_max, because the output before any sequence lies below 255 times the input before
// it and the rest of the room is at least 255 times what is left of the input, plus 64 — so the verdict and bytes are the same.
CJ_HD inline uint64_t lz4_slot_bytes(uint32_t word, uint32_t block_max) {
    const uint64_t c = word & 0x7FFFFFFFu;
    if (word & 0x80000000u) return c;
    return 255ull * c + 64ull < block_max ? 255ull * c + 64ull : block_max;
}

// cj_lz4_frame_decompress_bound: what the blocks can produce at most — a stored block its own size, a compressed block its slot
// (above) — or the first error of the headers.  The announced content size is attacker-controlled: it bounds the result from
// above, it never raises it (a 19-byte frame announcing 2^46 bytes used to make the caller allocate that; values >= 2^63
// turned into bogus negative "error codes").  Host (frame.hip) and device (batch_sizes.hip: one lane per frame).
CJ_HD inline int64_t lz4_frame_bound(const uint8_t* in, size_t n) {
    Lz4Header f;
    uint64_t total = 0;
    const int64_t err = lz4_frame_walk(in, n, f, [&](uint64_t, uint32_t w) { total += lz4_slot_bytes(w, f.block_max); return true; });
    if (err) return err;
    if (f.skippable) return 0;
    if (f.late_err) return f.late_err;
    if (f.csize && f.content_size < total) return (int64_t)f.content_size;
    return (int64_t)total;
}

// cj_snappy_frame_decompress_len: the decoded length from the chunk headers alone, or the first header-level error
CJ_HD inline int64_t snappy_frame_len(const uint8_t* in, size_t n) {
    uint64_t total = 0;
    const int64_t err = snappy_frame_walk(in, n, [](const SnapPiece&) {}, &total);
    return err ? err : (int64_t)total;
}

}  // namespace cj
