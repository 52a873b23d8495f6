// bgzf_grammar.hpp — the container grammar of BGZF, the blocked gzip of the SAM specification (§4.1): gzip members of at most 64 KiB
// laid end to end, each stating its own length in a `BC` extra subfield.  The walk hops from member to member without decoding and
// reports each one to a visitor; for the device (bgzf_batch.hip: one lane per stream) and, unchanged, for the host build under
// tests/hostsim.  Format rules only: the members themselves are the gzip member decoder's (deflate_wave.hpp).  Not part of the C-ABI.
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

constexpr uint32_t kBgzfPiece = 0xff00u;       // input bytes of a member this library writes: htslib's block size
constexpr uint32_t kBgzfHead = 18u;            // the header this library writes: the fixed 10 bytes, XLEN = 6, the BC subfield
constexpr uint32_t kBgzfMarker = 28u;          // the end-of-file marker: an empty member
constexpr uint32_t kBgzfMemberMin = 12u + 2u + 8u;      // + XLEN: fixed header and XLEN, an empty DEFLATE block, CRC32 and ISIZE

// Hops over the members of in[0, n); visit(member offset, member length, ISIZE) for each.  Returns 0 or the first error, the members
// before it visited.  Every read lies below n; a member is at least 28 bytes (XLEN >= 6), so the walk takes at most n / 26 + 1 hops.
// Bytes behind the last member — zero padding too, which Python's gzip tolerates — fail one of the checks of a member's head.
template <class V>
CJ_HD inline int64_t bgzf_walk(const uint8_t* in, size_t n, V&& visit) {
    size_t pos = 0;
    while (pos < n) {
        const uint8_t* p = in + pos;
        const size_t left = n - pos;
        if (left < 12u) return CJ_E_DEFLATE_EOF;
        const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
        if (left < 12u + xlen) return CJ_E_DEFLATE_EOF;
        if (p[0] != 31u || p[1] != 139u || p[2] != 8u || !(p[3] & 4u)) return CJ_E_DEFLATE_HEADER;
        const uint8_t* x = p + 12;
        size_t q = 0;
        bool have = false;
        uint32_t bsize = 0;
        while (q < xlen) {                                                   // SI1, SI2, SLEN, SLEN bytes
            if (xlen - q < 4u) return CJ_E_DEFLATE_HEADER;
            const size_t slen = (size_t)x[q + 2] | ((size_t)x[q + 3] << 8);
            if (slen > xlen - q - 4u) return CJ_E_DEFLATE_HEADER;
            if (!have && x[q] == 66u && x[q + 1] == 67u && slen == 2u) {     // the first BC subfield counts
                have = true;
                bsize = (uint32_t)x[q + 4] | ((uint32_t)x[q + 5] << 8);
            }
            q += 4u + slen;
        }
        if (!have) return CJ_E_DEFLATE_HEADER;
        const size_t len = (size_t)bsize + 1u;
        if (len < kBgzfMemberMin + xlen) return CJ_E_DEFLATE_HEADER;
        if (len > left) return CJ_E_DEFLATE_EOF;
        const uint8_t* t = p + len - 4;
        visit((uint64_t)pos, (uint32_t)len, (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24));
        pos += len;
    }
    return 0;
}

}  // namespace cj
