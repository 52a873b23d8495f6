// parquet_write.hpp — what the Parquet writer (parquet_write.hip) adds to parquet_grammar.hpp: the compact protocol
// WRITTEN — varints, zigzag, the PageHeader of one page with its fields in ascending order and short form —, a page's fields out of
// its row of the pages query's table, the table's rules, and the per-codec slot bound.  For the device (one lane writes a header) and,
// unchanged, for the host build under tests/hostsim, which holds pq_write_header to tests/parquet_model.py: header() byte for byte and
// reads every header back with pq_page_header.  Not part of the C-ABI.
//
// The header: 1 type, 2 uncompressed_page_size, 3 compressed_page_size, 4 crc (where asked for), then the page's own struct — 5
// DataPageHeader {1 num_values, 2 encoding, 3 definition_level_encoding, 4 repetition_level_encoding}, 7 DictionaryPageHeader
// {1 num_values, 2 encoding} (no is_sorted) or 8 DataPageHeaderV2 {1 num_values, 2 num_nulls, 3 num_rows, 4 encoding,
// 5 definition_levels_byte_length, 6 repetition_levels_byte_length, 7 is_compressed, always written} —, no Statistics.  Every field
// header is one byte, (delta << 4) | type, every I32 a zigzag varint of 1 .. 5 bytes.
// kPqMaxHeader = 57, a V2 page: type 2 bytes; the two sizes and the crc 6 each; the struct's header 1; num_values, num_nulls, num_rows
// 6 each; encoding 3 (it has 8 bits: a varint of 2 bytes at most); the two level lengths 6 each; is_compressed 1; the two stops 1 each.
#pragma once
#include "parquet_grammar.hpp"

namespace cj {

constexpr uint32_t kPqMaxHeader = 57;

// what a header states
struct PqFields {
    int32_t type, usize, csize;
    uint32_t crc;
    int32_t num_values, num_nulls, num_rows;
    int32_t encoding, def_enc, rep_enc;
    int32_t def_len, rep_len;
    bool has_crc, is_compressed;
};

// ---- the compact protocol, written -------------------------------------------------------------------------------------------------------
CJ_HD inline uint32_t pq_zigzag(int32_t x) { return ((uint32_t)x << 1) ^ (uint32_t)(x >> 31); }
CJ_HD inline uint32_t pq_varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }
// v at dst; returns the bytes written (pq_varint_len(v))
CJ_HD inline uint32_t pq_write_varint(uint8_t* dst, uint32_t v) {
    uint32_t k = 0;
    for (; v >= 0x80u; v >>= 7) dst[k++] = (uint8_t)(v | 0x80u);
    dst[k++] = (uint8_t)v;
    return k;
}

// The header's walk, once for the length (dst == nullptr) and once for the bytes: the two cannot disagree
CJ_HD inline uint32_t pq_header_walk(uint8_t* dst, const PqFields& f) {
    uint32_t k = 0;
    const auto put = [&](uint8_t b) { if (dst) dst[k] = b; k++; };
    const auto i32 = [&](uint32_t delta, int32_t v) {                     // an I32 field `delta` ids behind the last one
        put((uint8_t)(delta << 4 | 5u));
        const uint32_t z = pq_zigzag(v);
        k += dst ? pq_write_varint(dst + k, z) : pq_varint_len(z);
    };
    i32(1, f.type); i32(1, f.usize); i32(1, f.csize);
    if (f.has_crc) i32(1, (int32_t)f.crc);
    const uint32_t own = f.type == kPqDataPage ? 5u : f.type == kPqDictPage ? 7u : 8u;
    put((uint8_t)((own - (f.has_crc ? 4u : 3u)) << 4 | 12u));
    i32(1, f.num_values);
    if (own == 8u) { i32(1, f.num_nulls); i32(1, f.num_rows); }
    i32(1, f.encoding);
    if (own == 5u) { i32(1, f.def_enc); i32(1, f.rep_enc); }
    if (own == 8u) { i32(1, f.def_len); i32(1, f.rep_len); put(f.is_compressed ? 0x11u : 0x12u); }
    put(0); put(0);
    return k;
}
CJ_HD inline uint32_t pq_header_len(const PqFields& f) { return pq_header_walk(nullptr, f); }
// pq_header_len(f) bytes at dst, kPqMaxHeader at most; returns their number
CJ_HD inline uint32_t pq_write_header(uint8_t* dst, const PqFields& f) { return pq_header_walk(dst, f); }

// ---- the page table ------------------------------------------------------------------------------------------------------------------------
// The words of a row (cramjam_hip.h: the pages query) that the writer reads: 0 (low half the type, high half V2's num_nulls), 3, 5, 6
// (the encodings and bit 25) and 7.  0 or CJ_E_PARQUET_TABLE: a type outside {0, 2, 3}, a size that is no I32 >= 0, level lengths on a
// page that is not V2 or above the size.  csize, crc and is_compressed are the writer's to set.
constexpr uint32_t kPqRowHasCrc = 1u << 25;
CJ_HD inline int64_t pq_row_fields(const int64_t* w, PqFields& f) {
    f = PqFields{};
    const int64_t type = (int64_t)(int32_t)(uint32_t)w[0];
    if (type != kPqDataPage && type != kPqDictPage && type != kPqDataPageV2) return CJ_E_PARQUET_TABLE;
    if (w[3] < 0 || w[3] > 0x7fffffffll) return CJ_E_PARQUET_TABLE;
    const uint64_t def = (uint32_t)w[7], rep = (uint64_t)w[7] >> 32;
    if (type != kPqDataPageV2 && w[7] != 0) return CJ_E_PARQUET_TABLE;
    if (def + rep > (uint64_t)w[3]) return CJ_E_PARQUET_TABLE;
    f.type = (int32_t)type; f.usize = (int32_t)w[3];
    f.num_values = (int32_t)(uint32_t)w[5]; f.num_rows = type == kPqDataPageV2 ? (int32_t)((uint64_t)w[5] >> 32) : 0;
    f.num_nulls = type == kPqDataPageV2 ? (int32_t)((uint64_t)w[0] >> 32) : 0;
    f.encoding = (int32_t)(w[6] & 0xff); f.def_enc = (int32_t)((w[6] >> 8) & 0xff); f.rep_enc = (int32_t)((w[6] >> 16) & 0xff);
    f.def_len = (int32_t)def; f.rep_len = (int32_t)rep;
    f.has_crc = ((uint32_t)w[6] & kPqRowHasCrc) != 0u;
    return 0;
}

// ---- bounds --------------------------------------------------------------------------------------------------------------------------------
// What the codec's encoder may write for v bytes, at least cj::inner_bound(pq_inner(codec), v) (tests/test_parquet_write_model.py holds
// the two together): v + g(v) + K with g additive under floor — LZ4 v / 255 + 16, Snappy v / 6 + 32, gzip 10 (v / 65536) + 23,
// Zstandard 3 (v / 65536) + 13; UNCOMPRESSED v.  So the pages of any cut of n bytes into p pages need p K + n + g(n) at most.
CJ_HD inline uint64_t pq_slot_extra(int codec, uint64_t v) {
    return codec == kPqLz4Raw ? v / 255u : codec == kPqSnappy ? v / 6u : codec == kPqGzip ? 10u * (v >> 16) : codec == kPqZstd ? 3u * (v >> 16) : 0u;
}
CJ_HD inline uint64_t pq_slot_const(int codec) { return codec == kPqLz4Raw ? 16u : codec == kPqSnappy ? 32u : codec == kPqGzip ? 23u : codec == kPqZstd ? 13u : 0u; }
CJ_HD inline uint64_t pq_slot_bound(int codec, uint64_t v) { return v + pq_slot_extra(codec, v) + pq_slot_const(codec); }
// cj_parquet_compress_bound: every page a maximal header, its levels, and the slot bound of its values
CJ_HD inline uint64_t pq_chunk_bound(int codec, uint64_t n, uint64_t pages) { return pages * (kPqMaxHeader + pq_slot_const(codec)) + n + pq_slot_extra(codec, n); }

}  // namespace cj
