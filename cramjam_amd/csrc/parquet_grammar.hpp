// parquet_grammar.hpp — the page grammar of Parquet column chunks (parquet-format: "Data Pages", "Column chunks"; Thrift's compact
// protocol): a chunk is a run of pages that tile it exactly, each a compact-protocol PageHeader followed by compressed_page_size bytes.
// The walk hops from header to header without decoding a page and reports each page to a visitor; for the device (parquet_batch.hip:
// one lane per chunk) and, unchanged, for the host build under tests/hostsim.  Format rules only: the page bodies are the codecs'
// decoders'.  Not part of the C-ABI.
//
// The compact protocol as far as a header needs it.  A field header byte is (delta << 4) | type; delta 0: a zigzag varint field id
// follows; the byte 0 ends a struct.  Types: 1 / 2 bool true / false (no bytes behind a field header, one byte as an element), 3 one
// byte, 4 5 6 zigzag varints, 7 eight bytes, 8 a varint length and that many bytes, 9 / 10 list / set — (size << 4) | element type,
// a varint size behind it when the nibble is 15 —, 11 map — a varint size, then, unless it is 0, a key / value type byte —, 12 a
// struct.  Every other type is malformed, and so are a varint of more than 10 bytes and a container size that does not fit 31 bits.
// An I32 is the low 32 bits of the zigzag-decoded varint.  A field id this grammar does not know is skipped by its type, through at
// most kPqSkipDepth containers (structs, lists, sets, maps) inside one another, the field's own value counted; a known id must have
// its type; of a known id that appears twice the last one counts.  Every step — a field header, a value, an element — takes at least
// one byte, so a walk of n bytes makes at most n steps and never reads at or behind in + n.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/cramjam_hip.h"
#include "cj_codecs.hpp"

#if defined(__HIPCC__)
#define CJ_HD __host__ __device__
#else
#define CJ_HD
#endif

namespace cj {

// Parquet's CompressionCodec; LZO (3), BROTLI (4) and the deprecated Hadoop-framed LZ4 (5) are not read
constexpr int kPqUncompressed = 0, kPqSnappy = 1, kPqGzip = 2, kPqZstd = 6, kPqLz4Raw = 7;
CJ_HD inline bool pq_codec_ok(int c) { return c == kPqUncompressed || c == kPqSnappy || c == kPqGzip || c == kPqZstd || c == kPqLz4Raw; }
// the stream a coded page is (of a codec that pq_codec_ok accepts, but for kPqUncompressed: no page is coded)
constexpr Inner pq_inner(int c) { return c == kPqSnappy ? kInSnappyRaw : c == kPqGzip ? kInGzip : c == kPqLz4Raw ? kInLz4Raw : kInZstd; }

// PageType
constexpr int32_t kPqDataPage = 0, kPqIndexPage = 1, kPqDictPage = 2, kPqDataPageV2 = 3;
constexpr int kPqSkipDepth = 8;              // containers inside one another that the skip of one unknown field follows
constexpr size_t kPqPageWords = 8;           // int64 words of a page's row in the pages query's table

// One page as its header states it
struct PqPage {
    int32_t type, usize, csize;              // PageHeader 1, 2, 3
    uint32_t crc;                            // ... 4
    int32_t num_values, num_rows;            // the page's own struct; num_rows 0 outside V2
    int32_t encoding, def_enc, rep_enc;      // the level encodings 0 outside V1
    int32_t def_len, rep_len;                // V2: the level sections in front of the values; 0 elsewhere
    bool has_crc, is_compressed;             // is_compressed: V2's flag, true elsewhere
    uint64_t payload;                        // offset of the page's bytes in the chunk

    CJ_HD bool skipped() const { return type != kPqDataPage && type != kPqDictPage && type != kPqDataPageV2; }
    CJ_HD uint32_t levels() const { return (uint32_t)def_len + (uint32_t)rep_len; }
    // what the page adds to the decoded chunk: a page of a type that is not read adds nothing
    CJ_HD uint32_t decoded() const { return skipped() ? 0u : (uint32_t)usize; }
    // the codec sees the values section, and only where the file's codec is one and the page says it was applied
    CJ_HD bool coded(int codec) const { return !skipped() && codec != kPqUncompressed && is_compressed; }
    // the eight words of the pages query (cramjam_hip.h)
    CJ_HD void words(uint64_t out_at, int64_t* w) const {
        w[0] = type; w[1] = (int64_t)payload; w[2] = csize; w[3] = usize; w[4] = (int64_t)out_at;
        w[5] = (int64_t)((uint64_t)(uint32_t)num_values | (uint64_t)(uint32_t)num_rows << 32);
        w[6] = (int64_t)((uint32_t)(encoding & 0xff) | (uint32_t)(def_enc & 0xff) << 8 | (uint32_t)(rep_enc & 0xff) << 16 | (is_compressed ? 1u << 24 : 0u) |
                         (has_crc ? 1u << 25 : 0u));
        w[7] = (int64_t)((uint64_t)(uint32_t)def_len | (uint64_t)(uint32_t)rep_len << 32);
    }
};

// ---- the compact protocol ---------------------------------------------------------------------------------------------------------------
struct PqReader {
    const uint8_t* in;
    size_t n, pos;

    CJ_HD bool byte(uint8_t& b) {
        if (pos >= n) return false;
        b = in[pos++];
        return true;
    }
    CJ_HD bool varint(uint64_t& v) {
        v = 0;
        for (uint32_t k = 0; k < 10u; k++) {
            uint8_t b;
            if (!byte(b)) return false;
            v |= (uint64_t)(b & 0x7fu) << (7u * k);
            if (!(b & 0x80u)) return true;
        }
        return false;                                           // an 11th byte would follow
    }
    CJ_HD bool i32(int32_t& x) {
        uint64_t v;
        if (!varint(v)) return false;
        x = (int32_t)(uint32_t)((v >> 1) ^ (0u - (v & 1u)));
        return true;
    }
    CJ_HD bool size31(uint32_t& x) {
        uint64_t v;
        if (!varint(v) || v > 0x7fffffffull) return false;
        x = (uint32_t)v;
        return true;
    }
    CJ_HD bool hop(uint64_t k) {
        if (k > n - pos) return false;
        pos += (size_t)k;
        return true;
    }
    // a field header: type 0 = stop; id is the running field id of the struct
    CJ_HD bool field(uint32_t& type, int32_t& id) {
        uint8_t b;
        if (!byte(b)) return false;
        type = b & 15u;
        if (b == 0u) return true;
        if (type == 0u || type > 12u) return false;
        if ((b >> 4) != 0u) { id = (int32_t)((uint32_t)id + (b >> 4)); return true; }      // (wraps: a long-form id may stand at the top of the range)
        return i32(id);
    }

    // the value of an unknown field of `type`, skipped: an explicit stack of the open containers, no recursion.  A bool that is an element of
    // a list, set or map takes a byte; behind a field header its value is the type
    CJ_HD bool skip(uint32_t type) {
        struct Frame { uint64_t left; uint8_t kind, t0, t1; };   // kind 0 struct; 1 list / set of t0; 2 map: `left` keys (t0) and values (t1) in turn
        Frame st[kPqSkipDepth];
        int sp = 0;
        bool elem = false;
        for (;;) {
            // one value of `type`
            switch (type) {
            case 1: case 2: if (elem && !hop(1)) return false; break;
            case 3: if (!hop(1)) return false; break;
            case 4: case 5: case 6: { uint64_t v; if (!varint(v)) return false; break; }
            case 7: if (!hop(8)) return false; break;
            case 8: { uint32_t len; if (!size31(len) || !hop(len)) return false; break; }
            case 9: case 10: {
                uint8_t b;
                if (sp == kPqSkipDepth || !byte(b)) return false;
                uint32_t cnt = b >> 4;
                if (cnt == 15u && !size31(cnt)) return false;
                st[sp++] = Frame{cnt, 1, (uint8_t)(b & 15u), 0};
                break;
            }
            case 11: {
                uint32_t cnt;
                uint8_t b = 0;
                if (sp == kPqSkipDepth || !size31(cnt) || (cnt != 0u && !byte(b))) return false;
                st[sp++] = Frame{2ull * cnt, 2, (uint8_t)(b >> 4), (uint8_t)(b & 15u)};
                break;
            }
            case 12:
                if (sp == kPqSkipDepth) return false;
                st[sp++] = Frame{0, 0, 0, 0};
                break;
            default: return false;
            }
            // the next value of the innermost open container
            for (;;) {
                if (sp == 0) return true;
                Frame& f = st[sp - 1];
                if (f.kind == 0) {
                    int32_t id = 0;
                    if (!field(type, id)) return false;
                    if (type == 0u) { sp--; continue; }
                    elem = false;
                    break;
                }
                if (f.left == 0u) { sp--; continue; }
                type = (f.kind == 2 && (f.left & 1u)) ? f.t1 : f.t0;
                f.left--;
                elem = true;
                break;
            }
        }
    }
};

// One of the three page structs: `want[k]` is the compact type field k + 1 must have (0: none, the id is not known), `req` the ids that
// must appear (bit k = id k + 1); x[k] gets field k + 1.  A bool's value is its type.
CJ_HD inline bool pq_struct(PqReader& r, const uint8_t* want, int32_t nwant, uint32_t req, int32_t* x) {
    uint32_t seen = 0, type;
    int32_t id = 0;
    for (;;) {
        if (!r.field(type, id)) return false;
        if (type == 0u) break;
        if (id >= 1 && id <= nwant && want[id - 1] != 0u) {
            const bool isbool = want[id - 1] == 1u;
            if (isbool ? (type != 1u && type != 2u) : type != want[id - 1]) return false;
            if (isbool) x[id - 1] = type == 1u ? 1 : 0;
            else if (!r.i32(x[id - 1])) return false;
            seen |= 1u << (id - 1);
        } else if (!r.skip(type)) return false;
    }
    return (seen & req) == req;
}

// The header at r.pos: 0, r.pos behind it and pg filled but for pg.payload, or CJ_E_PARQUET_HEADER.  Where the payload ends is the
// caller's to check.  Page types 0, 2 and 3 must carry their own struct; a struct of another page type is parsed, held to its own
// rules and otherwise ignored.
CJ_HD inline int64_t pq_page_header(PqReader& r, PqPage& pg) {
    pg = PqPage{};
    pg.is_compressed = true;
    int32_t v1[4] = {}, dc[2] = {}, v2[7] = {};                 // DataPageHeader, DictionaryPageHeader, DataPageHeaderV2
    uint32_t seen = 0, type;                                    // bit k: PageHeader field k
    int32_t id = 0;
    for (;;) {
        if (!r.field(type, id)) return CJ_E_PARQUET_HEADER;
        if (type == 0u) break;
        if (id >= 1 && id <= 4) {
            int32_t v;
            if (type != 5u || !r.i32(v)) return CJ_E_PARQUET_HEADER;
            if (id == 1) pg.type = v; else if (id == 2) pg.usize = v; else if (id == 3) pg.csize = v; else pg.crc = (uint32_t)v;
        } else if (id == 5) {                                   // num_values, encoding, definition_level_encoding, repetition_level_encoding
            const uint8_t want[4] = {5, 5, 5, 5};
            if (type != 12u || !pq_struct(r, want, 4, 0xfu, v1)) return CJ_E_PARQUET_HEADER;
        } else if (id == 7) {                                   // num_values, encoding (is_sorted is skipped)
            const uint8_t want[2] = {5, 5};
            if (type != 12u || !pq_struct(r, want, 2, 0x3u, dc)) return CJ_E_PARQUET_HEADER;
        } else if (id == 8) {                                   // num_values, num_nulls, num_rows, encoding, the two level lengths, is_compressed
            const uint8_t want[7] = {5, 5, 5, 5, 5, 5, 1};
            v2[6] = 1;
            if (type != 12u || !pq_struct(r, want, 7, 0x3fu, v2)) return CJ_E_PARQUET_HEADER;
        } else if (!r.skip(type)) return CJ_E_PARQUET_HEADER;
        if (id >= 1 && id <= 8) seen |= 1u << id;
    }
    if ((seen & 0xeu) != 0xeu || pg.usize < 0 || pg.csize < 0) return CJ_E_PARQUET_HEADER;
    pg.has_crc = (seen & (1u << 4)) != 0u;
    if (pg.type == kPqDataPage) {
        if (!(seen & (1u << 5))) return CJ_E_PARQUET_HEADER;
        pg.num_values = v1[0]; pg.encoding = v1[1]; pg.def_enc = v1[2]; pg.rep_enc = v1[3];
    } else if (pg.type == kPqDictPage) {
        if (!(seen & (1u << 7))) return CJ_E_PARQUET_HEADER;
        pg.num_values = dc[0]; pg.encoding = dc[1];
    } else if (pg.type == kPqDataPageV2) {
        if (!(seen & (1u << 8))) return CJ_E_PARQUET_HEADER;
        pg.num_values = v2[0]; pg.num_rows = v2[2]; pg.encoding = v2[3]; pg.def_len = v2[4]; pg.rep_len = v2[5]; pg.is_compressed = v2[6] != 0;
        if (pg.def_len < 0 || pg.rep_len < 0) return CJ_E_PARQUET_HEADER;
        const uint64_t lv = (uint64_t)pg.def_len + (uint64_t)pg.rep_len;
        if (lv > (uint64_t)pg.csize || lv > (uint64_t)pg.usize) return CJ_E_PARQUET_HEADER;
    }
    return 0;
}

// Hops over the pages of in[0, n); visit(page) for each.  Returns 0 or CJ_E_PARQUET_HEADER, the pages before it visited.  Every read
// lies below n; a header takes at least one byte, so the walk makes at most n hops.
template <class V>
CJ_HD inline int64_t pq_walk(const uint8_t* in, size_t n, V&& visit) {
    PqReader r{in, n, 0};
    while (r.pos < n) {
        PqPage pg;
        const int64_t err = pq_page_header(r, pg);
        if (err != 0) return err;
        if ((uint64_t)pg.csize > n - r.pos) return CJ_E_PARQUET_HEADER;
        pg.payload = r.pos;
        visit(pg);
        r.pos += (size_t)pg.csize;
    }
    return 0;
}

}  // namespace cj
