// orc_grammar.hpp — the container grammar of ORC compression streams (ORC specification, "Compression"): every stream of a file with
// compression != NONE is a sequence of compression chunks, each a 3-byte little-endian header h and h >> 1 bytes — the codec's output
// for at most compressionBlockSize raw bytes, or (h & 1) those bytes as they are.  Nothing states a chunk's decoded length; there is
// no magic, no checksum and no end marker.  The walk hops from header to header without decoding and reports each chunk to a
// visitor; for the device (orc_batch.hip: one lane per stream) and, unchanged, for the host build under tests/hostsim.  Format rules
// only: the chunks themselves are the codecs' decoders'.  Not part of the C-ABI.
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

constexpr uint32_t kOrcHead = 3u;                     // the chunk header
constexpr uint32_t kOrcBlockMax = 1u << 23;           // a header's length field has 23 bits: no chunk, and so no block, is longer
constexpr uint32_t kOrcEncBlockMax = 262144u;         // the largest block this library writes (the encoders' pieces; ORC's default)

// PostScript.compression (CompressionKind); LZO (3), BROTLI (6) and NONE (0) are not read
constexpr int kOrcZlib = 1, kOrcSnappy = 2, kOrcLz4 = 4, kOrcZstd = 5;
CJ_HD inline bool orc_kind_ok(int kind) { return kind == kOrcZlib || kind == kOrcSnappy || kind == kOrcLz4 || kind == kOrcZstd; }
// the stream a compressed chunk is (of a kind that orc_kind_ok accepts)
constexpr Inner orc_inner(int kind) { return kind == kOrcZlib ? kInDeflateRaw : kind == kOrcSnappy ? kInSnappyRaw : kind == kOrcLz4 ? kInLz4Raw : kInZstd; }

// n + 3 * ceil(n / block_size): every piece as an original chunk.  Exact for incompressible input; an empty buffer is an empty stream.
CJ_HD inline uint64_t orc_bound(uint64_t n, uint64_t block_size) { return n + kOrcHead * ((n + block_size - 1u) / block_size); }

// Hops over the chunks of in[0, n); visit(offset of the chunk's bytes, their length, original) for each.  Returns 0 or the first
// error, the chunks before it visited.  Every read lies below n; a chunk takes at least its 3 header bytes, so the walk makes at most
// n / 3 hops.
template <class V>
CJ_HD inline int64_t orc_walk(const uint8_t* in, size_t n, V&& visit) {
    size_t pos = 0;
    while (pos < n) {
        if (n - pos < kOrcHead) return CJ_E_ORC_HEADER;
        const uint32_t h = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16);
        const size_t len = h >> 1;
        pos += kOrcHead;
        if (len > n - pos) return CJ_E_ORC_HEADER;
        visit((uint64_t)pos, (uint32_t)len, (h & 1u) != 0u);
        pos += len;
    }
    return 0;
}

}  // namespace cj
