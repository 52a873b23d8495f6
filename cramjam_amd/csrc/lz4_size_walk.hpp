// lz4_size_walk.hpp — the scalar statement of the LZ4 raw-block SIZE walk (cj_batch_sizes_device, batch_sizes.hip): what one lane
// decides per sequence when it only wants to know how long the block decodes, with output room that never runs out.  Plain
// per-thread code over a reader, for the kernels (lane per chunk through the LDS line rings, wavefront per chunk through the
// register window) and for a host build (tests/hostsim/sim_lz4_size_walk.cpp, under AddressSanitizer on exact-size buffers).
// Accept / reject rules: liblz4 1.10.0 LZ4_decompress_safe with a capacity of 255 * in_len + 64 (no capacity test can fail
// there: lz4_slot_bytes, frame_grammar.hpp), offset 0 rejected.  Differences to Lz4Grammar (parse_grammar.hpp):
// no capacity, lengths and the output position in 64 bits (in_len goes up to 0x7FFFFFF0: the size passes 32 bits long before
// it is judged), a run of length bytes is skipped as often as it goes on.
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

constexpr uint64_t kLz4InMax = 0x7FFFFFF0ull;       // LZ4_MAX_INPUT_SIZE's cousin of the safe decoder: a longer input is refused
constexpr uint64_t kLz4OutMax = 0x7E000000ull;      // the largest capacity the decoder accepts (lz4_block_prologue)

struct SizeSeq {
    uint64_t lit, mlen;        // literal bytes; match bytes (0 for the final sequence)
    uint32_t offset, next;     // match offset; position of the next token
    bool last;                 // the final, literal-only sequence: it consumed the input exactly
};

// Number of 0xFF bytes at g[ip ..] counted in whole 128-byte steps, staying 16 bytes clear of iend (the caller's byte loop
// finishes the run and keeps every bound it checks).  One length byte stands for 255 bytes: a match of gigabytes is
// megabytes of these.
CJ_HD inline uint32_t lz4_ff_run(const uint8_t* g, uint32_t ip, uint32_t iend) {
    uint32_t k = 0;
    while ((uint64_t)ip + k + 144u <= iend) {
        uint64_t w[16];
        __builtin_memcpy(w, g + ip + k, 128);
        uint64_t a = w[0];
        for (int i = 1; i < 16; i++) a &= w[i];
        if (a != ~0ull) break;
        k += 128u;
    }
    return k;
}

// One sequence at position ip, FROM THE INPUT BYTES ONLY.  rd(p) = the 4 bytes at p, little endian (bytes past iend may be
// anything); ff(p, iend) = a number of 0xFF bytes at p that may be skipped (lz4_ff_run, or 0).  False = a field or the
// sequence runs past the input.
template <class Rd, class Ff>
CJ_HD inline bool lz4_size_seq(const Rd& rd, const Ff& ff, uint32_t ip, uint32_t iend, SizeSeq& s) {
    const uint32_t t4 = rd(ip);
    const uint32_t token = t4 & 0xffu;
    ip += 1;
    uint64_t lit = token >> 4;
    if (lit == 15u) {
        if (ip + 15u >= iend) return false;
        uint32_t b = (t4 >> 8) & 0xffu;
        ip += 1; lit += b;
        if (ip + 15u > iend) return false;
        uint32_t streak = 0;
        while (b == 255u) {
            if (++streak == 8u) {
                const uint32_t k = ff(ip, iend);
                lit += 255ull * k; ip += k; streak = 0;
            }
            b = rd(ip) & 0xffu;
            ip += 1; lit += b;
            if (ip + 15u > iend) return false;
        }
    }
    s.lit = lit;
    const uint32_t rem_in = iend - ip;
    if ((uint64_t)rem_in < lit + 8u) {               // can only be the final sequence: it must consume the input exactly
        s.last = true; s.mlen = 0; s.offset = 0; s.next = iend;
        return (uint64_t)rem_in == lit;
    }
    s.last = false;
    ip += (uint32_t)lit;
    const uint32_t o4 = rd(ip);
    s.offset = o4 & 0xffffu;
    ip += 2;
    uint64_t mlen = token & 15u;
    if (mlen == 15u) {
        uint32_t b = (o4 >> 16) & 0xffu;
        ip += 1; mlen += b;
        if (ip + 4u > iend) return false;
        uint32_t streak = 0;
        while (b == 255u) {
            if (++streak == 8u) {
                const uint32_t k = ff(ip, iend);
                mlen += 255ull * k; ip += k; streak = 0;
            }
            b = rd(ip) & 0xffu;
            ip += 1; mlen += b;
            if (ip + 4u > iend) return false;
        }
    }
    s.mlen = mlen + 4u;
    s.next = ip;
    return true;
}

// ... and what needs the output position: the match must lie inside what was produced so far.  op moves on.
CJ_HD inline bool lz4_size_commit(const SizeSeq& s, uint64_t& op) {
    op += s.lit;
    if (s.last) return true;
    if (s.offset == 0u || (uint64_t)s.offset > op) return false;
    op += s.mlen;
    return true;
}
// ... of a block written against a dictionary (lz4_dict.hip): a match may also reach `hist` <= 65536 bytes behind the block's start.
// Only the dictionary's length enters, not its bytes.
CJ_HD inline bool lz4_size_commit(const SizeSeq& s, uint64_t& op, uint32_t hist) {
    op += s.lit;
    if (s.last) return true;
    if (s.offset == 0u || (uint64_t)s.offset > op + hist) return false;
    op += s.mlen;
    return true;
}

// the size of a block that walked to its end: no capacity the decoder accepts holds more than kLz4OutMax
CJ_HD inline int64_t lz4_size_verdict(uint64_t size) { return size > kLz4OutMax ? (int64_t)CJ_E_PREFIX_TOO_BIG : (int64_t)size; }

// The whole chain of a block that occupies positions [ip, iend) of the reader (ip > 0: a reader based below the block).
template <class Rd, class Ff>
CJ_HD inline int64_t lz4_size_walk(const Rd& rd, const Ff& ff, uint32_t ip, uint32_t iend) {
    if (ip >= iend) return CJ_E_CORRUPT;
    uint64_t op = 0;
    for (;;) {
        SizeSeq s;
        if (!lz4_size_seq(rd, ff, ip, iend, s) || !lz4_size_commit(s, op)) return CJ_E_CORRUPT;
        if (s.last) break;
        ip = s.next;
    }
    return lz4_size_verdict(op);
}
// ... with a dictionary of which `hist` bytes count
template <class Rd, class Ff>
CJ_HD inline int64_t lz4_size_walk(const Rd& rd, const Ff& ff, uint32_t ip, uint32_t iend, uint32_t hist) {
    if (ip >= iend) return CJ_E_CORRUPT;
    uint64_t op = 0;
    for (;;) {
        SizeSeq s;
        if (!lz4_size_seq(rd, ff, ip, iend, s) || !lz4_size_commit(s, op, hist)) return CJ_E_CORRUPT;
        if (s.last) break;
        ip = s.next;
    }
    return lz4_size_verdict(op);
}

}  // namespace cj
