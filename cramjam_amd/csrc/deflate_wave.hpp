// deflate_wave.hpp — the DEFLATE decoder of one wavefront (RFC 1951 behind no wrapper, RFC 1950 zlib or RFC 1952 gzip): one stream per
// wavefront, accept / reject rules of zlib's inflate.  Written like lz4_wave.hpp: it names only
//     InWindow, wave_copy, wave_match_copy, wave_order, CJ_LANES, lds_ld, lds_ld8, lds_add, lds_xor, out_ld8, LaneBytes
// of the wave-decoder contract: wave_lanes.hpp + cj_common.hpp implement it for the device,
// tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host (sim_deflate_decode.cpp), where
// the CPU tests hold the grammar, every copy's bounds and every table index to zlib.  Not part of the C-ABI.
//
// Mapping.  All stream state (bit buffer, positions, the symbol being decoded) is wave-uniform; the lanes build the Huffman tables
// and move the bytes.  A round is a run of up to 64 literals, lane k keeping literal k, stored in ONE step when a match, the
// end of the block or the 64th literal ends it; the match that ended it is then one wave_match_copy between two wave_order().  Stored
// blocks are a wave_copy.  Checksums are one lane-parallel pass over the finished output (crc32_lanes.hpp).
#pragma once
#include "crc32_lanes.hpp"
#include "wave_window.hpp"

namespace cj {

constexpr uint32_t kDfTabMask = 1023u;     // every table index is masked to this: the two tables hold 1024 entries each
constexpr uint32_t kDfLitRoot = 9u, kDfDistRoot = 6u, kDfClRoot = 7u;      // zlib's root widths
constexpr uint32_t kDfLitEnough = 852u, kDfDistEnough = 592u;              // zlib's ENOUGH_LENS / ENOUGH_DISTS for those roots
constexpr uint32_t kDfOutMax = 0x7E000000u;

// The wavefront's private LDS: 9.6 KiB (four wavefronts of a workgroup: 38.5 KiB of the 64 KiB of static LDS)
struct DeflateLds {
    uint32_t lit[1024];      // literal/length table: root of 512 entries, sub-tables behind it
    uint32_t dist[1024];     // distance table: root of 64, sub-tables behind it; the code-length code's table (128) while a header is read
    uint16_t code[320];      // canonical code of each symbol
    uint8_t lens[320];       // code lengths: literal/length symbols, then the distance symbols
    uint32_t count[16];      // symbols per code length
    uint32_t first[16];      // first canonical code of each length
    uint32_t acc[4];         // checksum accumulators
};

// A table entry: bits 0..3 = bits this level consumes, 4..6 = type, 8..11 = extra bits (sub-pointer: width of the sub-table),
// 16..31 = literal / base length / base distance / code-length symbol / sub-table offset.  0 — an entry nobody filled — is kDfInvalid
// with zero bits: it leaves the loop as CJ_E_DEFLATE_CORRUPT and is never "consumed".
constexpr uint32_t kDfInvalid = 0u, kDfLit = 1u, kDfLen = 2u, kDfEob = 3u, kDfSub = 4u, kDfDist = 5u, kDfCl = 6u;
__device__ __forceinline__ uint32_t df_entry(uint32_t type, uint32_t nbits, uint32_t extra, uint32_t val) { return (nbits & 15u) | (type << 4) | ((extra & 15u) << 8) | (val << 16); }
__device__ __forceinline__ uint32_t df_nbits(uint32_t e) { return e & 15u; }
__device__ __forceinline__ uint32_t df_type(uint32_t e) { return (e >> 4) & 7u; }
__device__ __forceinline__ uint32_t df_extra(uint32_t e) { return (e >> 8) & 15u; }
__device__ __forceinline__ uint32_t df_val(uint32_t e) { return e >> 16; }

__device__ __forceinline__ uint32_t df_bitrev(uint32_t v, uint32_t n) {      // the low n bits of v, reversed (1 <= n <= 15)
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32u - n);
}

// the order in which a dynamic block sends the lengths of the code-length code, five bits each in two constants (no table in memory)
constexpr uint64_t df_cl_pack(uint32_t from) {
    const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t w = 0;
    for (uint32_t k = 0; k < 12u && from + k < 19u; k++) w |= (uint64_t)o[from + k] << (5u * k);
    return w;
}
__device__ __forceinline__ uint32_t df_cl_order(uint32_t k) {
    constexpr uint64_t w0 = df_cl_pack(0), w1 = df_cl_pack(12);
    return (uint32_t)((k < 12u ? w0 >> (5u * k) : w1 >> (5u * (k - 12u))) & 31u);
}

// the entry of symbol s of an alphabet (kind = kDfLit / kDfDist / kDfCl) behind a code (or code tail) of nbits bits
__device__ __forceinline__ uint32_t df_symbol_entry(uint32_t kind, uint32_t s, uint32_t nbits) {
    if (kind == kDfCl) return df_entry(kDfCl, nbits, 0, s);
    if (kind == kDfDist) {
        if (s >= 30u) return df_entry(kDfInvalid, nbits, 0, 0);             // distance symbols 30 / 31
        const uint32_t extra = s < 4u ? 0u : (s >> 1) - 1u;
        const uint32_t base = s < 4u ? 1u + s : 1u + ((2u + (s & 1u)) << extra);
        return df_entry(kDfDist, nbits, extra, base);
    }
    if (s < 256u) return df_entry(kDfLit, nbits, 0, s);
    if (s == 256u) return df_entry(kDfEob, nbits, 0, 0);
    if (s >= 286u) return df_entry(kDfInvalid, nbits, 0, 0);                // literal/length symbols 286 / 287
    const uint32_t i = s - 257u;
    if (i < 8u) return df_entry(kDfLen, nbits, 0, 3u + i);
    if (i == 28u) return df_entry(kDfLen, nbits, 0, 258u);
    const uint32_t extra = (i >> 2) - 1u;
    return df_entry(kDfLen, nbits, extra, 3u + ((4u + (i & 3u)) << extra));
}

// Build the table of one alphabet from L->lens[at, at + nsym), all 64 lanes together: per-length counts (one LDS add per symbol), the
// set's check by zlib's rules (inflate_table: over-subscribed is an error; incomplete is legal only for the two data alphabets when
// every code has length 1; no code at all is legal and decodes nothing), first codes, each symbol's canonical code (lane l walks the
// symbols of length l in order), the sub-tables' places (lane p looks at root prefix p), and then every lane fills the entries of
// its own symbols.  Returns false for a set zlib refuses.  `enough`: the entries zlib proves sufficient; a set that wanted more is refused
// too (it cannot pass the checks before it; the test keeps the fill inside the table without relying on that proof).
__device__ __forceinline__ bool df_build(DeflateLds* L, uint32_t* tab, uint32_t kind, uint32_t root, uint32_t enough, uint32_t at, uint32_t nsym) {
    CJ_LANES(lane) { if (lane < 16u) L->count[lane] = 0u; }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) {
            const uint32_t l = L->lens[at + s];
            if (l != 0u) lds_add(&L->count[l], 1u);
        }
    }
    wave_order();
    uint32_t max = 0;
    int32_t left = 1;
    for (uint32_t l = 1; l <= 15u; l++) {
        const uint32_t c = lds_ld(&L->count[l]);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return false;                                          // over-subscribed
        if (c != 0u) max = l;
    }
    if (left > 0 && max != 0u && (kind == kDfCl || max != 1u)) return false;   // incomplete
    // what an index nobody fills decodes to: with a complete set there is none; with one code of length 1 or no code at all zlib's
    // table holds "invalid code" entries of one bit (the code-length alphabet without a code: symbol 0 in one bit, as inflate reads it)
    uint32_t blank = kDfInvalid;
    if (left > 0) blank = (kind == kDfCl) ? df_entry(kDfCl, 1, 0, 0) : df_entry(kDfInvalid, 1, 0, 0);
    CJ_LANES(lane) {
        if (lane >= 1u && lane < 16u) {
            uint32_t code = 0;
            for (uint32_t j = 1; j < lane; j++) code = (code + L->count[j]) << 1;
            L->first[lane] = code;
        }
        for (uint32_t i = lane; i <= kDfTabMask; i += 64u) tab[i] = blank;
    }
    wave_order();
    // canonical codes: lane l numbers the symbols of length l in symbol order
    CJ_LANES(lane) {
        if (lane >= 1u && lane <= max) {
            uint32_t next = L->first[lane];
            for (uint32_t s = 0; s < nsym; s++)
                if (L->lens[at + s] == lane) L->code[s] = (uint16_t)next++;
        }
    }
    // sub-tables (zlib's shape): root prefix p >= P0 leads to codes longer than root; its sub-table spans the longest code below it.
    // Codes grow with their length, so the lengths l in use above root start at prefixes P(l) that only grow, prefix p belongs to the
    // longest l with P(l) <= p, and the sub-tables lie in prefix order behind the root.
    uint32_t total = 1u << root;
    if (max > root) {
        const uint32_t p0 = lds_ld(&L->first[root + 1u]) >> 1;
        const uint32_t np = (1u << root) - p0;
        uint32_t prev_l = 0, prev_p = 0;
        for (uint32_t l = root + 1u; l <= max; l++) {                        // the space in front of prefix 2^root = all of it
            if (lds_ld(&L->count[l]) == 0u) continue;
            const uint32_t P = lds_ld(&L->first[l]) >> (l - root);
            if (prev_l != 0u) total += (P - prev_p) << (prev_l - root);
            prev_l = l; prev_p = P;
        }
        total += ((1u << root) - prev_p) << (prev_l - root);
        if (total > enough || p0 >= (1u << root)) return false;
        CJ_LANES(lane) {
            for (uint32_t k = lane; k < np; k += 64u) {
                const uint32_t p = p0 + k;
                uint32_t off = 1u << root, ml = 0, pl = 0, pp = 0;
                for (uint32_t l = root + 1u; l <= max; l++) {
                    if (L->count[l] == 0u) continue;
                    const uint32_t P = L->first[l] >> (l - root);
                    const uint32_t a = p < P ? p : P, b = p < pp ? p : pp;
                    if (pl != 0u) off += (a - b) << (pl - root);
                    if (P <= p) ml = l;
                    pl = l; pp = P;
                }
                off += (p - (p < pp ? p : pp)) << (pl - root);
                tab[df_bitrev(p, root)] = df_entry(kDfSub, root, ml - root, off);
            }
        }
    }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) {
            const uint32_t l = L->lens[at + s];
            if (l == 0u) continue;
            const uint32_t rc = df_bitrev(L->code[s], l);
            if (l <= root) {
                const uint32_t e = df_symbol_entry(kind, s, l);
                for (uint32_t i = rc; i < (1u << root); i += 1u << l) tab[i] = e;
            } else {
                const uint32_t sub = tab[rc & ((1u << root) - 1u)];
                const uint32_t off = df_val(sub), sb = df_extra(sub), tail = l - root;
                const uint32_t e = df_symbol_entry(kind, s, tail);
                if (df_type(sub) == kDfSub && tail <= sb)
                    for (uint32_t i = rc >> root; i < (1u << sb); i += 1u << tail) tab[(off + i) & kDfTabMask] = e;
            }
        }
    }
    wave_order();
    return true;
}

// ---- the bit reader: a 64-bit buffer of VALID bits, refilled from the register window --------------------------------------------
// cnt counts only bits of the stream: the bytes a refill takes are clipped to in_len and masked, so no bit behind in_len is ever
// used; a caller that needs k bits and finds cnt < k after a refill has reached the end of the input (CJ_E_DEFLATE_EOF).
struct DfBits {
    InWindow w;
    uint32_t ip;       // next byte to load, relative to w.base
    uint32_t cnt;      // valid bits in buf
    uint64_t buf;
    __device__ __forceinline__ void init(const uint8_t* in, uint32_t n) {
        ip = window_open(w, in, n);
        cnt = 0; buf = 0;
    }
    // afterwards cnt >= 33, or every bit of the input is in the buffer
    __device__ __forceinline__ void refill() {
        if (cnt <= 32u && ip < w.iend) {
            const uint32_t left = w.iend - ip, take = left < 4u ? left : 4u;
            w.ensure(ip);
            uint32_t v = w.fetch32(ip);
            if (take < 4u) v &= (1u << (8u * take)) - 1u;
            buf |= (uint64_t)v << cnt;
            cnt += 8u * take;
            ip += take;
        }
    }
    __device__ __forceinline__ uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }      // k <= 16
    __device__ __forceinline__ void drop(uint32_t k) { buf >>= k; cnt -= k; }
    // k <= 32 bits, or false at the end of the input
    __device__ __forceinline__ bool get(uint32_t k, uint32_t& v) {
        refill();
        if (cnt < k) return false;
        v = (uint32_t)(buf & ((1ull << k) - 1ull));
        drop(k);
        return true;
    }
    __device__ __forceinline__ void align() { drop(cnt & 7u); }
    // the position of the next unread byte (the buffer holds whole bytes only: after align()), with the buffer emptied
    __device__ __forceinline__ uint32_t rewind() { ip -= cnt >> 3; cnt = 0; buf = 0; return ip; }
    __device__ __forceinline__ bool at_end() const { return cnt == 0u && ip >= w.iend; }
};

// One symbol of a two-level table.  0: ok (e = its entry, the code's bits dropped); otherwise the error.  The root's bits are looked
// up as they are (bits the input does not have read as 0): as in inflate, an entry counts once the input holds all of ITS bits.
__device__ __forceinline__ int32_t df_symbol(DfBits& b, const uint32_t* tab, uint32_t root, uint32_t& e) {
    e = lds_ld(&tab[b.peek(root)]);
    uint32_t nb = df_nbits(e);
    if (nb > b.cnt) return CJ_E_DEFLATE_EOF;
    if (df_type(e) == kDfSub) {
        const uint32_t sb = df_extra(e);
        e = lds_ld(&tab[(df_val(e) + (((uint32_t)(b.buf >> root)) & ((1u << sb) - 1u))) & kDfTabMask]);
        nb = root + df_nbits(e);
        if (nb > b.cnt) return CJ_E_DEFLATE_EOF;
        if (df_type(e) == kDfSub) return CJ_E_DEFLATE_CORRUPT;
    }
    if (df_type(e) == kDfInvalid || nb == 0u) return CJ_E_DEFLATE_CORRUPT;
    b.drop(nb);
    return 0;
}

// The walk of one stream (deflate_wave_decode below).  The capacity's rule is inflate's with ONE byte of room behind the capacity, the
// rule the verdicts of the tests are computed by: the first byte that does not fit is not written but kept (`over`, its value in
// over_byte: a later match may copy it, and the checksums cover it), the walk goes on without output, and whatever needs a SECOND
// byte of room returns CJ_E_OUT_TOO_SMALL — so an error that inflate meets between those two bytes is that error, as it is for zlib.
template <int WRAP, bool SIZE>
__device__ __forceinline__ int64_t deflate_wave_walk(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, DeflateLds* L,
                                                     const uint32_t* crc_adv, const uint32_t* crc_xpow8, bool& over) {
    const uint64_t room = SIZE ? kDfOutMax : cap;
    const int64_t full = SIZE ? CJ_E_PREFIX_TOO_BIG : CJ_E_OUT_TOO_SMALL;
    uint32_t over_byte = 0;
    DfBits b;
    b.init(in, n);
    uint32_t v = 0;

    // ---- the wrapper's header -------------------------------------------------------------------------------------------------
    if (WRAP == CJ_DEFLATE_ZLIB) {
        uint32_t cmf, flg;
        if (!b.get(8, cmf) || !b.get(8, flg)) return CJ_E_DEFLATE_EOF;
        if (((cmf << 8) | flg) % 31u != 0u || (cmf & 15u) != 8u || (cmf >> 4) > 7u) return CJ_E_DEFLATE_HEADER;
        if (flg & 0x20u) {                                                   // FDICT: inflate reads the id, then asks for the dictionary
            if (!b.get(32, v)) return CJ_E_DEFLATE_EOF;
            return CJ_E_DEFLATE_HEADER;
        }
    }
    if (WRAP == CJ_DEFLATE_GZIP) {
        // every header byte enters the header's CRC-32 (bytewise; used only with FHCRC)
        uint32_t hcrc = 0xFFFFFFFFu, flg = 0;
        bool eof = false;
        auto byte = [&]() -> uint32_t {
            uint32_t x = 0;
            if (!b.get(8, x)) { eof = true; return 0u; }
            hcrc ^= x;
            for (int k = 0; k < 8; k++) hcrc = (hcrc >> 1) ^ ((hcrc & 1u) ? kCrc32Poly : 0u);
            return x;
        };
        const uint32_t id1 = byte(), id2 = byte();
        if (eof) return CJ_E_DEFLATE_EOF;
        if (id1 != 0x1fu || id2 != 0x8bu) return CJ_E_DEFLATE_HEADER;
        const uint32_t cm = byte();
        flg = byte();
        if (eof) return CJ_E_DEFLATE_EOF;
        if (cm != 8u || (flg & 0xe0u)) return CJ_E_DEFLATE_HEADER;
        for (int k = 0; k < 6; k++) byte();                                  // MTIME, XFL, OS
        if (eof) return CJ_E_DEFLATE_EOF;
        if (flg & 4u) {                                                      // FEXTRA
            uint32_t xlen = byte();
            xlen |= byte() << 8;
            for (uint32_t k = 0; k < xlen && !eof; k++) byte();              // (each byte() consumes input or sets eof: at most in_len turns)
            if (eof) return CJ_E_DEFLATE_EOF;
        }
        for (uint32_t field = 8u; field <= 16u; field <<= 1) {               // FNAME, FCOMMENT: zero-terminated
            if (!(flg & field)) continue;
            while (byte() != 0u && !eof) {}
            if (eof) return CJ_E_DEFLATE_EOF;
        }
        if (flg & 2u) {                                                      // FHCRC: the low 16 bits of the CRC-32 of what came before
            const uint32_t want = ~hcrc & 0xffffu;
            uint32_t got;
            if (!b.get(16, got)) return CJ_E_DEFLATE_EOF;
            if (got != want) return CJ_E_DEFLATE_HEADER;
        }
    }

    // ---- the blocks -------------------------------------------------------------------------------------------------------------
    uint32_t op = 0;           // bytes decoded, the round's pending literals included
    uint32_t pend = 0;         // literals of the round that the lanes still hold
    LaneBytes lits;
    uint32_t last = 0;
    do {
        uint32_t hdr;
        if (!b.get(3, hdr)) return CJ_E_DEFLATE_EOF;
        last = hdr & 1u;
        const uint32_t type = hdr >> 1;
        if (type == 3u) return CJ_E_DEFLATE_CORRUPT;
        if (type == 0u) {
            // stored: LEN, ~LEN, then LEN bytes from the next byte boundary
            b.align();
            if (!b.get(32, v)) return CJ_E_DEFLATE_EOF;
            const uint32_t len = v & 0xffffu;
            if (len != ((v >> 16) ^ 0xffffu)) return CJ_E_DEFLATE_CORRUPT;
            const uint32_t src = b.rewind(), have = b.w.iend - src;
            // stream order, as inflate copies min(LEN, input, room): the byte that does not fit comes before the byte that is missing
            const uint32_t avail = len < have ? len : have;
            if ((uint64_t)avail > room - op) {
                const uint32_t fits = (uint32_t)(room - op);
                if (SIZE || over || avail - fits >= 2u || len != avail) return full;
                wave_copy(out + op, b.w.base + src, fits);                   // the block ends with the one byte kept behind the capacity
                op += fits;
                b.w.anchor(src + fits);
                over_byte = b.w.fetch32(src + fits) & 0xffu;
                over = true;
                b.ip = src + len;
                continue;
            }
            if (over && len != 0u) return full;
            if (have < len) return CJ_E_DEFLATE_EOF;
            if (!SIZE) wave_copy(out + op, b.w.base + src, len);
            op += len;
            b.ip = src + len;
            continue;
        }
        if (type == 1u) {
            CJ_LANES(lane) {
                for (uint32_t s = lane; s < 320u; s += 64u) L->lens[s] = s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < 288u ? 8u : 5u;
            }
            wave_order();
            if (!df_build(L, L->lit, kDfLit, kDfLitRoot, kDfLitEnough, 0u, 288u) || !df_build(L, L->dist, kDfDist, kDfDistRoot, kDfDistEnough, 288u, 32u))
                return CJ_E_DEFLATE_CORRUPT;
        } else {
            if (!b.get(14, v)) return CJ_E_DEFLATE_EOF;
            const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = (v >> 10) + 4u;
            if (nlen > 286u || ndist > 30u) return CJ_E_DEFLATE_CORRUPT;
            // the code-length code: ncode lengths of 3 bits in the format's order; lane k holds the length of symbol k
            CJ_LANES(lane) { if (lane < 19u) L->lens[lane] = 0u; }
            wave_order();
            for (uint32_t k = 0; k < ncode; k++) {
                if (!b.get(3, v)) return CJ_E_DEFLATE_EOF;
                const uint32_t o = df_cl_order(k);
                const uint32_t len3 = v;
                CJ_LANES(lane) { if (lane == o) L->lens[lane] = (uint8_t)len3; }
            }
            wave_order();
            if (!df_build(L, L->dist, kDfCl, kDfClRoot, 128u, 0u, 19u)) return CJ_E_DEFLATE_CORRUPT;
            // the code lengths of both alphabets, run-length coded
            uint32_t have = 0, prev = 0;
            const uint32_t want = nlen + ndist;
            while (have < want) {                                            // every turn consumes at least one bit or leaves
                b.refill();
                uint32_t e;
                // the symbol and its repeat count count only together (inflate: NEEDBITS(here.bits + 2 / 3 / 7))
                const uint32_t e0 = lds_ld(&L->dist[b.peek(kDfClRoot) & 127u]);
                const uint32_t s0 = df_val(e0);
                const uint32_t need = df_nbits(e0) + (df_type(e0) != kDfCl ? 0u : s0 == 16u ? 2u : s0 == 17u ? 3u : s0 == 18u ? 7u : 0u);
                if (need > b.cnt) return CJ_E_DEFLATE_EOF;
                const int32_t rc = df_symbol(b, L->dist, kDfClRoot, e);
                if (rc != 0) return rc;
                if (df_type(e) != kDfCl) return CJ_E_DEFLATE_CORRUPT;
                const uint32_t s = df_val(e);
                uint32_t rep = 1, len = s;
                if (s >= 16u) {
                    if (s == 16u) {
                        if (have == 0u) return CJ_E_DEFLATE_CORRUPT;
                        len = prev; rep = 3u + b.peek(2); b.drop(2);
                    } else if (s == 17u) {
                        len = 0; rep = 3u + b.peek(3); b.drop(3);
                    } else {
                        len = 0; rep = 11u + b.peek(7); b.drop(7);
                    }
                    if (have + rep > want) return CJ_E_DEFLATE_CORRUPT;
                }
                // literal/length lengths at lens[0, nlen), distance lengths at lens[288, 288 + ndist)
                CJ_LANES(lane) {
                    for (uint32_t j = lane; j < rep; j += 64u) {
                        const uint32_t idx = have + j;
                        L->lens[idx < nlen ? idx : 288u + (idx - nlen)] = (uint8_t)len;
                    }
                }
                have += rep;
                prev = len;
            }
            wave_order();
            if (lds_ld8(&L->lens[256]) == 0u) return CJ_E_DEFLATE_CORRUPT;   // no end-of-block code
            if (!df_build(L, L->lit, kDfLit, kDfLitRoot, kDfLitEnough, 0u, nlen) || !df_build(L, L->dist, kDfDist, kDfDistRoot, kDfDistEnough, 288u, ndist))
                return CJ_E_DEFLATE_CORRUPT;
        }

        // ---- the symbols of a compressed block ------------------------------------------------------------------------------------
        // This loop ends: a turn either returns, breaks at the end-of-block code, or has df_symbol drop the bits of an entry, and
        // df_symbol drops at least ONE bit or reports an error (an entry of zero bits, which only an unfilled index holds, is
        // CJ_E_DEFLATE_CORRUPT, and every index is masked into the wavefront's own table).  The input has 8 * in_len bits, the reader
        // never invents one (DfBits), so after at most 8 * in_len turns the reader is empty and the next turn returns
        // CJ_E_DEFLATE_EOF.  The loops around it are bounded the same way: a block header takes 3 bits, a code length at least one.
        for (;;) {
            b.refill();
            uint32_t e;
            int32_t rc = df_symbol(b, L->lit, kDfLitRoot, e);
            if (rc != 0) return rc;
            const uint32_t t = df_type(e);
            if (t == kDfLit) {
                if ((uint64_t)op >= room) {
                    if (SIZE || over) return full;
                    over = true;
                    over_byte = df_val(e);
                    continue;
                }
                if (!SIZE) {
                    lits.put(pend, df_val(e));
                    if (++pend == 64u) { lits.flush(out + (op + 1u - 64u), 64u); pend = 0; }
                }
                op += 1u;
                continue;
            }
            if (!SIZE && pend != 0u) { lits.flush(out + (op - pend), pend); pend = 0; }
            if (t == kDfEob) break;
            if (t != kDfLen) return CJ_E_DEFLATE_CORRUPT;
            uint32_t len = df_val(e), x = df_extra(e);
            if (x > b.cnt) return CJ_E_DEFLATE_EOF;
            len += b.peek(x); b.drop(x);
            b.refill();
            rc = df_symbol(b, L->dist, kDfDistRoot, e);
            if (rc != 0) return rc;
            if (df_type(e) != kDfDist) return CJ_E_DEFLATE_CORRUPT;
            uint32_t d = df_val(e);
            x = df_extra(e);
            if (x > b.cnt) return CJ_E_DEFLATE_EOF;
            d += b.peek(x); b.drop(x);
            if (over) return full;                                           // (inflate asks for room before it looks at the distance's reach)
            if (d > op) return CJ_E_DEFLATE_CORRUPT;                         // the symbol's own validity before its fit
            if ((uint64_t)len > room - op) {
                if (SIZE || (uint64_t)len - (room - op) >= 2u) return full;
                wave_order();                                                // all but its last byte fit: that one is kept
                wave_match_copy(out + op, d, len - 1u);
                wave_order();
                op += len - 1u;
                over_byte = out_ld8(out + (op - d));
                over = true;
                continue;
            }
            if (!SIZE) {
                wave_order();
                wave_match_copy(out + op, d, len);
                wave_order();
            }
            op += len;
        }
    } while (!last);

    // ---- the end of the stream --------------------------------------------------------------------------------------------------
    b.align();
    if (WRAP == CJ_DEFLATE_ZLIB) {
        uint32_t sum;                                                        // big-endian in the stream
        if (!b.get(32, sum)) return CJ_E_DEFLATE_EOF;
        if (!SIZE) {
            wave_order();
            CJ_LANES(lane) { if (lane < 2u) L->acc[lane] = 0u; }
            wave_order();
            CJ_LANES(lane) {
                uint32_t a, s2;
                adler32_lane(out, op, lane, [](const uint8_t* q) { uint32_t x; __builtin_memcpy(&x, q, 4); return x; }, a, s2);
                lds_add(&L->acc[0], a);
                lds_add(&L->acc[1], s2);
            }
            wave_order();
            uint32_t a = (1u + lds_ld(&L->acc[0])) % 65521u, s2 = (op % 65521u + lds_ld(&L->acc[1])) % 65521u;
            if (over) { a = (a + over_byte) % 65521u; s2 = (s2 + a) % 65521u; }
            if (__builtin_bswap32(sum) != ((s2 << 16) | a)) return CJ_E_DEFLATE_CHECKSUM;
        }
    }
    if (WRAP == CJ_DEFLATE_GZIP) {
        uint32_t crc, isize;
        if (!b.get(32, crc)) return CJ_E_DEFLATE_EOF;
        if (!SIZE) {
            wave_order();
            CJ_LANES(lane) { if (lane == 0u) L->acc[2] = 0u; }
            wave_order();
            CJ_LANES(lane) {
                lds_xor(&L->acc[2], crc32_lane(out, op, lane, crc_adv, crc_xpow8, [](const uint8_t* q) { uint32_t x; __builtin_memcpy(&x, q, 4); return x; }));
            }
            wave_order();
            uint32_t reg = lds_ld(&L->acc[2]);
            if (over) {
                reg ^= over_byte;
                for (int k = 0; k < 8; k++) reg = (reg >> 1) ^ ((reg & 1u) ? kCrc32Poly : 0u);
            }
            if (crc != ~reg) return CJ_E_DEFLATE_CHECKSUM;
        }
        if (!b.get(32, isize)) return CJ_E_DEFLATE_EOF;
        if (!SIZE && isize != op + (over ? 1u : 0u)) return CJ_E_DEFLATE_CHECKSUM;
    }
    if (!b.at_end()) return CJ_E_DEFLATE_TRAILING;
    return (int64_t)op;
}

// Decode one stream (wave-uniform arguments): n <= 0x7FFFFFF0 bytes at in, cap <= 0x7E000000 bytes at out.  Returns the decoded length
// or CJ_E_*.  SIZE: the size query — the same walk with every store and both checksums compiled out; out and cap are not used, a
// total above 0x7E000000 is CJ_E_PREFIX_TOO_BIG.  crc_adv / crc_xpow8: crc32_lanes.hpp's tables (gzip decode only).
template <int WRAP, bool SIZE>
__device__ __forceinline__ int64_t deflate_wave_decode(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, DeflateLds* L,
                                                       const uint32_t* crc_adv, const uint32_t* crc_xpow8) {
    bool over = false;
    const int64_t r = deflate_wave_walk<WRAP, SIZE>(in, n, out, cap, L, crc_adv, crc_xpow8, over);
    // with a byte kept behind the capacity the stream's end, the input's end and bytes behind the stream all mean that it did not fit
    if (over && (r >= 0 || r == CJ_E_DEFLATE_EOF || r == CJ_E_DEFLATE_TRAILING)) return CJ_E_OUT_TOO_SMALL;
    return r;
}

}  // namespace cj
