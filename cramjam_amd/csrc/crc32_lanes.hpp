// crc32_lanes.hpp — CRC-32 (IEEE 802.3, reflected 0xEDB88320: gzip's) of one piece by 64 lanes, the sibling of crc32c_lanes.hpp;
// behind it Adler-32 (zlib's) by the same lanes: the two checksums of the DEFLATE decoder and encoder.
//
// The same linearity argument and the same lane mapping as there: lane l owns dwords l, l + 64, l + 128, ... of the piece (one
// coalesced 256 B wave load per step), advances its register over the 256 bytes of the others with four table lookups and its last
// dword to the end of the piece with one GF(2) multiplication by x^(8 * bytes_to_end); the XOR of the 64 results is the CRC register
// (lane 0 starts from 0xFFFFFFFF, the others from 0).  crc32c_lanes.hpp and its users stay as they are; only the polynomial differs,
// and it is a constant of that file.  Plain integer code for host and device: tests/hostsim runs it for lanes 0..63 inside the
// DEFLATE decoder's host build against zlib's crc32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define CJ_HD32 __host__ __device__
#else
#define CJ_HD32
#endif

namespace cj {

constexpr uint32_t kCrc32Poly = 0xEDB88320u;

// a * b mod P in the reflected representation (x^0 is bit 31)
CJ_HD32 constexpr uint32_t gf_mul_ieee(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrc32Poly : 0u);
    }
    return p;
}

constexpr uint32_t kCrc32TailEntries = 260;   // x^(8n), n = 0 .. 259 (a lane's last dword starts at most 259 bytes before the end)

struct Crc32Tables {
    uint32_t adv256[4][256];              // adv256[j][b] = (b << 8j) * x^(8*256)
    uint32_t xpow8[kCrc32TailEntries];    // x^(8n) mod P
};

constexpr Crc32Tables make_crc32_tables() {
    Crc32Tables t{};
    t.xpow8[0] = 0x80000000u;
    for (uint32_t n = 1; n < kCrc32TailEntries; n++) t.xpow8[n] = gf_mul_ieee(t.xpow8[n - 1], 0x00800000u);   // * x^8
    const uint32_t m = t.xpow8[256];
    for (uint32_t j = 0; j < 4; j++)
        for (uint32_t b = 0; b < 256; b++) t.adv256[j][b] = gf_mul_ieee(b << (8u * j), m);
    return t;
}

// One lane's share of p[0, len).  adv: the 4 x 256 table (LDS on the device); xpow8: the tail multipliers.  Returns the lane's
// contribution to the (un-inverted) CRC register.
template <class Ld32>
CJ_HD32 inline uint32_t crc32_lane(const uint8_t* p, uint32_t len, uint32_t lane, const uint32_t* adv, const uint32_t* xpow8, Ld32 ld32) {
    uint32_t s = lane == 0u ? 0xFFFFFFFFu : 0u;
    uint32_t pos = 4u * lane;
    while (pos < len && len - pos >= 4u) {
        const uint32_t v = s ^ ld32(p + pos);
        if (len - pos <= 256u) return gf_mul_ieee(v, xpow8[len - pos]);   // last dword of this lane: 4 .. 256 bytes to the end
        s = adv[v & 0xffu] ^ adv[256u + ((v >> 8) & 0xffu)] ^ adv[512u + ((v >> 16) & 0xffu)] ^ adv[768u + (v >> 24)];
        pos += 256u;
    }
    if (pos < len) {                                                      // 1..3 trailing bytes
        uint32_t d = 0;
        for (uint32_t k = 0; k < len - pos; k++) d |= (uint32_t)p[pos + k] << (8u * k);
        return gf_mul_ieee(s ^ d, xpow8[len - pos]);
    }
    return s;   // the lane owns nothing behind its last full step: s is 0 (or, for lane 0 of an empty piece, the init value)
}

// ---- Adler-32, lane-parallel ----------------------------------------------------------------------------------------------------------
// adler = 1 + sum(x_i), sum2 = n + sum((n - i) * x_i), both mod 65521.  Lane l owns dwords l, l + 64, ... as above and
// adds its bytes with their weights (n - i) mod 65521; the lanes' sums are added in LDS.  a, s2: this lane's two sums, below 65521.
template <class Ld32>
CJ_HD32 inline void adler32_lane(const uint8_t* p, uint32_t n, uint32_t lane, Ld32 ld32, uint32_t& a, uint32_t& s2) {
    constexpr uint32_t M = 65521u;
    uint64_t sa = 0, sb = 0;
    uint32_t pos = 4u * lane;
    uint32_t w = pos < n ? (n - pos) % M : 0u;           // weight of the byte at pos
    while (pos < n && n - pos >= 4u) {
        const uint32_t v = ld32(p + pos);
        const uint32_t b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
        sa += b0 + b1 + b2 + b3;
        sb += (uint64_t)(b0 + b1 + b2 + b3) * (w + M) - (b1 + 2u * b2 + 3u * b3);      // weights w, w - 1, w - 2, w - 3 (mod M)
        pos += 256u;
        w = w >= 256u ? w - 256u : w + M - 256u;
    }
    if (pos < n) {
        for (uint32_t k = 0; k < n - pos; k++) { sa += p[pos + k]; sb += (uint64_t)p[pos + k] * (n - pos - k); }
    }
    a = (uint32_t)(sa % M);
    s2 = (uint32_t)(sb % M);
}

}  // namespace cj
