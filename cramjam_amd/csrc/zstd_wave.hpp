// zstd_wave.hpp — the Zstandard decoder of one wavefront (RFC 8878 frames, no dictionary): one chunk of one or more frames per
// wavefront, accept / reject rules of libzstd's one-shot ZSTD_decompress (1.4.x).  Written like deflate_wave.hpp: it
// names only
//     InWindow, wave_copy, wave_match_copy, wave_order, CJ_LANES, lds_ld, lds_add, lds_or, in_ld8, in_ld32 (the Huffman streams: one
//     lane per stream), slot_st8 (the literal slot), out_ld8, out_rd32 (XXH64), LaneBytes
// of the wave-decoder contract: wave_lanes.hpp + cj_common.hpp implement it for the device,
// tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host (sim_zstd_decode.cpp).  Not part of the C-ABI.
//
// Mapping.  All grammar state is wave-uniform: frame and block headers, the FSE table descriptions, the sequences' backward
// bitstream (an exact model of libzstd's 64-bit BIT_DStream_t, so that a stream that over-reads gets libzstd's verdict) and the three
// repeat offsets.  The lanes build the Huffman table, move the bytes and take the Huffman streams: a block has one or four, so one or
// four lanes decode literals into the wavefront's literal slot in global memory (128 KiB + 32) while the other lanes idle — the
// format's limit for one block.  A stream's end follows the one of libzstd's two Huffman decoders that libzstd would take (zs_huf_select_x2).  Each sequence is a wave_copy of its literals and a wave_match_copy, as the LZ4 and DEFLATE wave
// decoders do; the END of a block's sequence stream follows the one of libzstd's two sequence decoders that libzstd would take (a
// frame with a window above 16 MiB may get the one that decodes ahead: the sequences section below).  XXH64 runs over the finished frame: the four accumulators on four lanes.
//
// The size query (SIZE) is the same walk without stores, literal decoding and checksum.  It does NOT report:
//   - CJ_E_ZSTD_CHECKSUM (no output exists to sum)
//   - in a frame WITH Frame_Content_Size: anything inside a block (the blocks' headers are walked, their bodies skipped, the size is
//     the header's): every CJ_E_ZSTD_CORRUPT cause but a reserved block type, a content size that the blocks do not produce, and the
//     CJ_E_ZSTD_SRC_SIZE of a sequences header that its block cuts short
//   - in a frame without it: what only the literals' decoding finds (a bad Huffman tree description or stream, Treeless literals
//     without a table); literal counts come from the literals header, match lengths from the decoded sequences, and offsets and
//     literal overruns are still checked
// A chunk the decoder refuses for one of these may get a size or a later error from the query; every other verdict is the decoder's.
#pragma once
#include "wave_window.hpp"

namespace cj {

constexpr uint32_t kZsBlockMax = 131072u;
constexpr uint32_t kZsSlotBytes = kZsBlockMax + 32u;       // the literal slot of a stream in flight (three of four streams may run 2 bytes over)
constexpr uint32_t kZsOutMax = 0x7E000000u;
constexpr uint32_t kZsLL = 0u, kZsML = 512u, kZsOF = 1024u;   // the three sequence tables inside ZstdLds::fse

// The wavefront's private LDS: 10.0 KiB (four wavefronts of a workgroup: 39.9 KiB of the 64 KiB of static LDS).  fse, huf, weights
// and the table logs live across the blocks of a frame: that is what Repeat and Treeless mean.
struct ZstdLds {
    uint32_t fse[1280];      // LL (512) | ML (512) | OF (256): symbol | bits << 8 | next-state base << 16
    uint8_t huf[4096];       // Huffman symbol by the next hlog bits (libzstd reads up to 12); its bits = hlog + 1 - weights[symbol];
                             // the weights' own FSE table (64 words) while a tree description is read
    uint8_t weights[256];
    uint16_t work[256];      // normalized counts / next-state counters of a table being built; the symbols sorted by weight
    uint32_t cnt[16], rstart[16], sbase[16];      // per Huffman weight: symbols, first table cell, first place in work[]
    uint32_t acc[8];         // XXH64 accumulators (lo, hi)
    uint32_t flag;           // a lane's Huffman stream broke the rules
};

__device__ __forceinline__ uint32_t zs_highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      // v != 0

// ---- wave-uniform reads of the input through the register window ------------------------------------------------------------------
// Positions are relative to w.base.  Callers read only below iend; what a 32-bit read brings from beyond is masked off.
struct ZsIn {
    InWindow w;
    __device__ __forceinline__ void init(const uint8_t* in, uint32_t n) { window_open(w, in, n); }
    __device__ __forceinline__ uint32_t f32(uint32_t pos) {               // reading forward
        if (pos - w.wpos > 500u) w.anchor(pos);
        return w.fetch32(pos);
    }
    __device__ __forceinline__ uint32_t b32(uint32_t pos) {               // reading backward (the bitstreams)
        if (pos - w.wpos > 500u) w.anchor(pos > 480u ? pos - 480u : 0u);
        return w.fetch32(pos);
    }
    __device__ __forceinline__ uint32_t f8(uint32_t pos) { return f32(pos) & 0xffu; }
    // k <= 4 bytes little-endian
    __device__ __forceinline__ uint32_t fle(uint32_t pos, uint32_t k) { const uint32_t v = f32(pos); return k >= 4u ? v : v & ((1u << (8u * k)) - 1u); }
    __device__ __forceinline__ uint64_t b64(uint32_t pos) { const uint32_t lo = b32(pos), hi = b32(pos + 4u); return ((uint64_t)hi << 32) | lo; }
};

// ---- libzstd's BIT_DStream_t, bit for bit (64-bit build): container, bitsConsumed, ptr, the reload rules ------------------------
constexpr uint32_t kZsUnfinished = 0u, kZsEndOfBuffer = 1u, kZsCompleted = 2u, kZsOverflow = 3u;
struct ZsBitD {
    uint64_t c;
    uint32_t bc, ptr, start;
    __device__ __forceinline__ bool init(ZsIn& in, uint32_t s, uint32_t size) {
        start = s;
        if (size < 1u) return false;
        const uint32_t last = in.b32(s + size - 1u) & 0xffu;
        if (last == 0u) return false;
        bc = 8u - zs_highbit(last);
        if (size >= 8u) {
            ptr = s + size - 8u;
            c = in.b64(ptr);
        } else {
            ptr = s;
            c = in.b64(s) & ((1ull << (8u * size)) - 1ull);
            bc += (8u - size) * 8u;
        }
        return true;
    }
    __device__ __forceinline__ uint32_t reload(ZsIn& in) {
        if (bc > 64u) return kZsOverflow;
        if (ptr >= start + 8u) { ptr -= bc >> 3; bc &= 7u; c = in.b64(ptr); return kZsUnfinished; }
        if (ptr == start) return bc < 64u ? kZsEndOfBuffer : kZsCompleted;
        uint32_t nb = bc >> 3, res = kZsUnfinished;
        if (nb > ptr - start) { nb = ptr - start; res = kZsEndOfBuffer; }
        ptr -= nb; bc -= nb * 8u;
        c = in.b64(ptr);
        return res;
    }
    __device__ __forceinline__ uint32_t read(uint32_t nb) {                 // BIT_readBits (BIT_getMiddleBits): nb may be 0
        const uint64_t v = (c >> ((64u - bc - nb) & 63u)) & ((1ull << nb) - 1ull);
        bc += nb;
        return (uint32_t)v;
    }
    __device__ __forceinline__ uint32_t read_fast(uint32_t nb) {            // BIT_readBitsFast: nb >= 1
        const uint64_t v = (c << (bc & 63u)) >> ((64u - nb) & 63u);
        bc += nb;
        return (uint32_t)v;
    }
};

// ---- the codes' base values and extra bits ----------------------------------------------------------------------------------------
__device__ __forceinline__ void zs_ll_code(uint32_t s, uint32_t& base, uint32_t& bits) {
    static const uint8_t kBits[20] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    static const uint32_t kBase[20] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    if (s < 16u) { base = s; bits = 0u; return; }
    s = s - 16u < 19u ? s - 16u : 19u;
    base = kBase[s]; bits = kBits[s];
}
__device__ __forceinline__ void zs_ml_code(uint32_t s, uint32_t& base, uint32_t& bits) {
    static const uint8_t kBits[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    static const uint32_t kBase[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    if (s < 32u) { base = s + 3u; bits = 0u; return; }
    s = s - 32u < 20u ? s - 32u : 20u;
    base = kBase[s]; bits = kBits[s];
}
__device__ __forceinline__ int32_t zs_default_norm(uint32_t which, uint32_t s) {
    static const int8_t kLL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    static const int8_t kOF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    static const int8_t kML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    return which == 0u ? kLL[s < 36u ? s : 35u] : which == 1u ? kOF[s < 29u ? s : 28u] : kML[s < 53u ? s : 52u];
}

// ---- FSE ------------------------------------------------------------------------------------------------------------------------
// FSE_readNCount (libzstd 1.4.7 and later) over in[at, at + hb): the normalized counts of symbols 0 .. max_sv (at most 255) into
// L->work as int16.  Returns the header's length, or 0 for a description libzstd refuses; log and nsym (symbols described) come back.
__device__ __forceinline__ uint32_t zs_read_ncount(ZsIn& in, ZstdLds* L, uint32_t at, uint32_t hb, uint32_t max_sv, uint32_t& log, uint32_t& nsym) {
    const uint32_t eff = hb < 8u ? 8u : hb;                                  // a header below 8 bytes is read from a zero-padded copy
    auto rd32 = [&](uint32_t ip) -> uint32_t {                               // ip + 4 <= eff
        if (ip >= hb) return 0u;
        const uint32_t have = hb - ip;
        return in.fle(at + ip, have < 4u ? have : 4u);
    };
    const uint32_t max1 = max_sv + 1u;
    CJ_LANES(lane) { for (uint32_t s = lane; s < 256u; s += 64u) L->work[s] = 0u; }
    wave_order();
    uint32_t ip = 0, bit_stream = rd32(0);
    uint32_t nb = (bit_stream & 15u) + 5u;
    if (nb > 15u) return 0u;
    bit_stream >>= 4;
    int32_t bit_count = 4;
    log = nb;
    int32_t remaining = (1 << nb) + 1, threshold = 1 << nb;
    nb++;
    uint32_t charnum = 0;
    bool prev0 = false;
    auto advance = [&]() {
        if (ip + 7u <= eff || ip + (uint32_t)(bit_count >> 3) + 4u <= eff) { ip += (uint32_t)(bit_count >> 3); bit_count &= 7; }
        else { bit_count -= (int32_t)(8u * (eff - 4u - ip)); bit_count &= 31; ip = eff - 4u; }
        bit_stream = rd32(ip) >> bit_count;
    };
    for (;;) {                                                               // every turn describes a symbol or leaves: at most 256 turns
        if (prev0) {
            uint32_t repeats = (uint32_t)__builtin_ctz(~bit_stream | 0x80000000u) >> 1;
            while (repeats >= 12u) {
                charnum += 36u;
                if (charnum > 512u) return 0u;                               // (far beyond max1: libzstd ends the same way, later)
                if (ip + 7u <= eff) ip += 3u;
                else { bit_count -= (int32_t)(8u * (eff - 7u - ip)); bit_count &= 31; ip = eff - 4u; }
                bit_stream = rd32(ip) >> bit_count;
                repeats = (uint32_t)__builtin_ctz(~bit_stream | 0x80000000u) >> 1;
            }
            charnum += 3u * repeats;
            bit_stream >>= 2u * repeats;
            bit_count += (int32_t)(2u * repeats);
            charnum += bit_stream & 3u;
            bit_count += 2;
            if (charnum >= max1) break;
            advance();
        }
        const int32_t max = (2 * threshold - 1) - remaining;
        int32_t count;
        if ((bit_stream & (uint32_t)(threshold - 1)) < (uint32_t)max) {
            count = (int32_t)(bit_stream & (uint32_t)(threshold - 1));
            bit_count += (int32_t)nb - 1;
        } else {
            count = (int32_t)(bit_stream & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= max;
            bit_count += (int32_t)nb;
        }
        count--;
        remaining -= count >= 0 ? count : 1;
        const uint32_t at_sym = charnum++, cv = (uint32_t)count & 0xffffu;
        CJ_LANES(lane) { if (lane == 0u) L->work[at_sym & 255u] = (uint16_t)cv; }
        prev0 = count == 0;
        if (remaining < threshold) {
            if (remaining <= 1) break;
            nb = zs_highbit((uint32_t)remaining) + 1u;
            threshold = 1 << (nb - 1u);
        }
        if (charnum >= max1) break;
        advance();
    }
    wave_order();
    if (remaining != 1 || charnum > max1 || bit_count > 32) return 0u;
    nsym = charnum;
    ip += (uint32_t)((bit_count + 7) >> 3);
    if (ip > hb) return 0u;
    return ip;
}

// The decoding table of `nsym` normalized counts in L->work, libzstd's construction (FSE_buildDTable / ZSTD_buildFSETable): the cells
// of the "less than one" symbols from the top, the spread with its skip rule, then the next-state numbering in cell order.  The skip
// rule makes a cell's symbol depend on every cell before it, so ONE lane walks the table (at most 512 cells, twice).  log <= 9 and the
// table has 1 << log cells at tab.
__device__ __forceinline__ void zs_fse_build(ZstdLds* L, uint32_t* tab, uint32_t log, uint32_t nsym) {
    CJ_LANES(lane) {
        if (lane == 0u) {
            const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
            uint32_t high = size;                                            // the cells [high, size) are taken
            for (uint32_t s = 0; s < nsym; s++)
                if (L->work[s] == 0xffffu && high != 0u) tab[--high] = s;
            uint32_t pos = 0;
            for (uint32_t s = 0; s < nsym && high != 0u; s++) {
                const uint32_t c = L->work[s];
                if (c == 0xffffu) continue;
                for (uint32_t i = 0; i < c && i < size; i++) {
                    tab[pos & mask] = s;
                    pos = (pos + step) & mask;
                    while (pos >= high) pos = (pos + step) & mask;
                }
            }
            for (uint32_t s = 0; s < nsym; s++)
                if (L->work[s] == 0xffffu) L->work[s] = 1u;
            for (uint32_t u = 0; u < size; u++) {
                const uint32_t s = tab[u] & 255u;
                uint32_t next = L->work[s];
                L->work[s] = (uint16_t)(next + 1u);
                if (next == 0u) next = 1u;
                const uint32_t nbits = log - zs_highbit(next);
                tab[u] = s | (nbits << 8) | ((((next << nbits) - size) & 0xffffu) << 16);
            }
        }
    }
    wave_order();
}

// one table of the sequences section (ZSTD_buildSeqTable).  which: 0 LL, 1 OF, 2 ML.  mode: the two bits of the modes byte.  pos
// advances over what the mode reads.  valid: a table of an earlier block exists (Repeat).  false: libzstd's corruption_detected
__device__ __forceinline__ bool zs_seq_table(ZsIn& in, ZstdLds* L, uint32_t which, uint32_t mode, uint32_t& pos, uint32_t end, bool valid, uint32_t& tlog) {
    uint32_t* tab = &L->fse[which == 0u ? kZsLL : which == 1u ? kZsOF : kZsML];
    const uint32_t max_sv = which == 0u ? 35u : which == 1u ? 31u : 52u, max_log = which == 1u ? 8u : 9u;
    if (mode == 3u) return valid;
    if (mode == 1u) {
        if (pos >= end) return false;
        const uint32_t s = in.f8(pos);
        if (s > max_sv) return false;
        pos += 1u;
        CJ_LANES(lane) { if (lane == 0u) tab[0] = s; }
        wave_order();
        tlog = 0u;
        return true;
    }
    uint32_t nsym;
    if (mode == 0u) {
        nsym = which == 0u ? 36u : which == 1u ? 29u : 53u;
        tlog = which == 1u ? 5u : 6u;
        CJ_LANES(lane) { if (lane < nsym) L->work[lane] = (uint16_t)zs_default_norm(which, lane); }
        wave_order();
    } else {
        const uint32_t h = zs_read_ncount(in, L, pos, end - pos, max_sv, tlog, nsym);
        if (h == 0u || tlog > max_log) return false;
        pos += h;
    }
    zs_fse_build(L, tab, tlog, nsym);
    return true;
}

// ---- Huffman ----------------------------------------------------------------------------------------------------------------------
// HUF_readStats + HUF_readDTableX1 over in[at, at + size): the weights into L->weights, the table into L->huf.  Returns the
// description's length (0: refused), hlog the table's width.
__device__ __forceinline__ uint32_t zs_huf_read(ZsIn& in, ZstdLds* L, uint32_t at, uint32_t size, uint32_t& hlog) {
    if (size == 0u) return 0u;
    uint32_t isize = in.f8(at), osize;
    CJ_LANES(lane) { for (uint32_t s = lane; s < 256u; s += 64u) L->weights[s] = 0u; }
    wave_order();
    if (isize >= 128u) {                                                     // direct: four bits a weight
        osize = isize - 127u;
        isize = (osize + 1u) / 2u;
        if (isize + 1u > size) return 0u;
        for (uint32_t k = 0; k < isize; k += 4u) {
            const uint32_t v = in.fle(at + 1u + k, isize - k < 4u ? isize - k : 4u);
            CJ_LANES(lane) {
                if (lane < 8u && k * 2u + lane < osize) L->weights[k * 2u + lane] = (uint8_t)((v >> (8u * (lane >> 1) + ((lane & 1u) ? 0u : 4u))) & 15u);
            }
        }
        wave_order();
    } else {                                                                 // FSE-compressed (FSE_decompress_wksp, two interleaved states)
        if (isize + 1u > size) return 0u;
        uint32_t wlog, nsym;
        const uint32_t h = zs_read_ncount(in, L, at + 1u, isize, 255u, wlog, nsym);
        if (h == 0u || wlog > 6u) return 0u;
        // libzstd (1.4.7 and later) decodes the weights in a workspace sized for 12 symbols at log 6 (HUF_READ_STATS_WORKSPACE_SIZE_U32 =
        // FSE_DECOMPRESS_WKSP_SIZE_U32(6, 11) = 89 words) and refuses a description whose table (1 + cells) and build space (two bytes a
        // symbol described, a byte a cell, 8) need more: above 12 symbols at log 6, above 92 at log 5
        if (1u + (1u << wlog) + ((2u * nsym + (1u << wlog) + 8u + 3u) >> 2) > 89u) return 0u;
        uint32_t* wtab = reinterpret_cast<uint32_t*>(L->huf);
        zs_fse_build(L, wtab, wlog, nsym);
        ZsBitD b;
        if (!b.init(in, at + 1u + h, isize - h)) return 0u;
        uint32_t st[2];
        st[0] = b.read(wlog); b.reload(in);
        st[1] = b.read(wlog); b.reload(in);
        osize = 0;
        for (uint32_t k = 0;; k ^= 1u) {                                     // libzstd's tail loop: a symbol, its bits, until the stream over-reads
            if (osize > 253u) return 0u;
            uint32_t e = lds_ld(&wtab[st[k] & 63u]);
            uint32_t sym = e & 255u;
            st[k] = (e >> 16) + b.read((e >> 8) & 255u);
            const uint32_t o0 = osize++;
            CJ_LANES(lane) { if (lane == 0u) L->weights[o0] = (uint8_t)sym; }
            if (b.reload(in) == kZsOverflow) {
                e = lds_ld(&wtab[st[k ^ 1u] & 63u]);
                sym = e & 255u;
                const uint32_t o1 = osize++;
                CJ_LANES(lane) { if (lane == 0u) L->weights[o1] = (uint8_t)sym; }
                break;
            }
        }
        wave_order();
    }
    // the weights' statistics, the implied last weight, libzstd's checks
    CJ_LANES(lane) { if (lane < 16u) L->cnt[lane] = 0u; if (lane == 0u) L->flag = 0u; }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < osize; s += 64u) {
            const uint32_t wt = L->weights[s];
            if (wt >= 12u) lds_or(&L->flag, 1u);
            else lds_add(&L->cnt[wt], 1u);
        }
    }
    wave_order();
    if (lds_ld(&L->flag) != 0u) return 0u;
    uint32_t total = 0;
    for (uint32_t wt = 1; wt < 12u; wt++) total += lds_ld(&L->cnt[wt]) << (wt - 1u);
    if (total == 0u) return 0u;
    hlog = zs_highbit(total) + 1u;
    if (hlog > 12u) return 0u;
    const uint32_t rest = (1u << hlog) - total;
    if (rest == 0u || (rest & (rest - 1u)) != 0u) return 0u;
    const uint32_t lastw = zs_highbit(rest) + 1u;
    CJ_LANES(lane) { if (lane == 0u) { L->weights[osize] = (uint8_t)lastw; L->cnt[lastw] += 1u; } }
    wave_order();
    const uint32_t c1 = lds_ld(&L->cnt[1]);
    if (c1 < 2u || (c1 & 1u)) return 0u;
    const uint32_t nsym = osize + 1u, log = hlog;
    // the cells of weight w start at rstart[w] and are 1 << (w - 1) per symbol, the symbols in symbol order: lane w sorts its symbols
    // into work[sbase[w] ..], then every lane fills cells
    CJ_LANES(lane) {
        if (lane >= 1u && lane <= 12u) {
            uint32_t cell = 0, place = 0;
            for (uint32_t wt = 1; wt < lane; wt++) { cell += L->cnt[wt] << (wt - 1u); place += L->cnt[wt]; }
            L->rstart[lane] = cell;
            L->sbase[lane] = place;
        }
    }
    wave_order();
    CJ_LANES(lane) {
        if (lane >= 1u && lane <= log) {
            uint32_t place = L->sbase[lane];
            for (uint32_t s = 0; s < nsym; s++)
                if (L->weights[s] == lane) L->work[place++ & 255u] = (uint16_t)s;
        }
    }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t u = lane; u < (1u << log); u += 64u) {
            uint32_t wt = 1;
            for (uint32_t k = 2; k <= log; k++) if (L->cnt[k] != 0u && u >= L->rstart[k]) wt = k;
            if (L->cnt[wt] == 0u) continue;                                  // (cannot be: the cells of all weights add up to 1 << log)
            L->huf[u] = (uint8_t)L->work[(L->sbase[wt] + ((u - L->rstart[wt]) >> (wt - 1u))) & 255u];
        }
    }
    wave_order();
    return isize + 1u;
}

// One Huffman stream, a lane's own work: `count` symbols of src[0, size) into dst.  libzstd's rule (HUF_decodeStreamX1 and
// BIT_endOfDStream): the stream holds exactly the bits of its symbols behind the final-bit marker.
__device__ __forceinline__ bool zs_huf_stream(const ZstdLds* L, uint32_t log, const uint8_t* src, uint32_t size, uint8_t* dst, uint32_t count) {
    if (size == 0u) return false;
    const uint32_t last = in_ld8(src + size - 1u);
    if (last == 0u) return false;
    uint32_t pos = size - 1u, cnt = zs_highbit(last);
    uint64_t acc = last & ((1u << cnt) - 1u);
    const uint32_t mask = (1u << log) - 1u;
    for (uint32_t i = 0; i < count; i++) {
        if (cnt <= 32u) {
            if (pos >= 4u) { pos -= 4u; acc = (acc << 32) | in_ld32(src + pos); cnt += 32u; }
            else while (pos > 0u) { pos--; acc = (acc << 8) | in_ld8(src + pos); cnt += 8u; }
        }
        const uint32_t idx = (cnt >= log ? (uint32_t)(acc >> (cnt - log)) : (uint32_t)(acc << (log - cnt))) & mask;
        const uint32_t sym = L->huf[idx & 4095u];
        const uint32_t nb = log + 1u - L->weights[sym];
        if (nb > cnt) return false;
        cnt -= nb;
        acc &= (1ull << cnt) - 1ull;
        slot_st8(dst + i, sym);
    }
    return cnt == 0u && pos == 0u;
}

// libzstd has a second Huffman decoder, of two symbols per lookup of 12 bits (HUF_decodeStreamX2), and takes it where its timing table
// says so (HUF_selectDecoder, below).  Both read the same symbols from a well-formed stream; they differ at a damaged stream's END: a
// lookup yields a pair when both codes fit 12 bits, the segment's last symbol, when it is left over alone, is taken from a lookup
// whose bits are only charged up to the stream's end when the lookup was a pair, and with no bit left that lookup reads the
// container's top (the stream's first 8 bytes) and counts only as a pair.  This is that decoder for one stream.
__device__ __forceinline__ bool zs_huf_stream_x2(const ZstdLds* L, uint32_t log, const uint8_t* src, uint32_t size, uint8_t* dst, uint32_t count) {
    if (size == 0u) return false;
    const uint32_t last = in_ld8(src + size - 1u);
    if (last == 0u) return false;
    uint32_t pos = size - 1u, cnt = zs_highbit(last);
    uint64_t acc = last & ((1u << cnt) - 1u);
    // the entry of a 12-bit lookup v: its first symbol, the second when both codes fit, the bits of what it holds
    auto entry = [&](uint32_t v, uint32_t& s1, uint32_t& s2, uint32_t& nbits) -> uint32_t {
        s1 = L->huf[(v >> (12u - log)) & 4095u];
        const uint32_t nb1 = log + 1u - L->weights[s1];
        s2 = L->huf[(((v << nb1) & 4095u) >> (12u - log)) & 4095u];
        const uint32_t nb2 = log + 1u - L->weights[s2];
        if (nb1 + nb2 <= 12u) { nbits = nb1 + nb2; return 2u; }
        nbits = nb1;
        return 1u;
    };
    uint32_t p = 0, s1, s2, nbits;
    while (p < count) {
        if (cnt <= 32u) {
            if (pos >= 4u) { pos -= 4u; acc = (acc << 32) | in_ld32(src + pos); cnt += 32u; }
            else while (pos > 0u) { pos--; acc = (acc << 8) | in_ld8(src + pos); cnt += 8u; }
        }
        const uint32_t v = (cnt >= 12u ? (uint32_t)(acc >> (cnt - 12u)) : (uint32_t)(acc << (12u - cnt))) & 4095u;
        if (p + 2u <= count) {
            const uint32_t len = entry(v, s1, s2, nbits);
            if (nbits > cnt) return false;
            slot_st8(dst + p, s1);
            if (len == 2u) slot_st8(dst + p + 1u, s2);
            p += len;
            cnt -= nbits;
            acc &= (1ull << cnt) - 1ull;
            continue;
        }
        // the last symbol, alone (HUF_decodeLastSymbolX2)
        if (cnt == 0u) {
            uint64_t c = 0;
            for (uint32_t k = 0; k < 8u && k < size; k++) c |= (uint64_t)in_ld8(src + k) << (8u * k);
            if (entry((uint32_t)(c >> 52), s1, s2, nbits) != 2u) return false;
            slot_st8(dst + p, s1);
            return pos == 0u;
        }
        const uint32_t len = entry(v, s1, s2, nbits);
        slot_st8(dst + p, s1);
        if (len == 2u) return nbits >= cnt && pos == 0u;
        return nbits == cnt && pos == 0u;
    }
    return cnt == 0u && pos == 0u;
}

// HUF_selectDecoder: true = the double-symbol decoder, for dst_size literals out of c_size bytes (libzstd's timing table)
__device__ __forceinline__ bool zs_huf_select_x2(uint32_t dst_size, uint32_t c_size) {
    static const uint16_t kT[16][4] = {{0, 0, 1, 1},       {0, 0, 1, 1},       {38, 130, 1313, 74},  {448, 128, 1353, 74}, {556, 128, 1353, 74}, {714, 128, 1418, 74},
                                       {883, 128, 1437, 74}, {897, 128, 1515, 75}, {926, 128, 1613, 75}, {947, 128, 1729, 77}, {1107, 128, 2083, 81}, {1177, 128, 2379, 87},
                                       {1242, 128, 2415, 93}, {1349, 128, 2644, 106}, {1455, 128, 2422, 124}, {722, 128, 1891, 145}};
    const uint32_t q = c_size >= dst_size ? 15u : (uint32_t)((uint64_t)c_size * 16u / dst_size), d256 = dst_size >> 8;
    const uint32_t t0 = kT[q][0] + kT[q][1] * d256;
    uint32_t t1 = kT[q][2] + kT[q][3] * d256;
    t1 += t1 >> 3;
    return t1 < t0;
}

// ---- XXH64 ------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kXxP1 = 0x9E3779B185EBCA87ull, kXxP2 = 0xC2B2AE3D27D4EB4Full, kXxP3 = 0x165667B19E3779F9ull, kXxP4 = 0x85EBCA77C2B2AE63ull,
                   kXxP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ uint64_t zs_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
__device__ __forceinline__ uint64_t zs_xx_round(uint64_t acc, uint64_t v) { return zs_rotl(acc + v * kXxP2, 31) * kXxP1; }
__device__ __forceinline__ uint64_t zs_xx_merge(uint64_t h, uint64_t v) { return (h ^ zs_xx_round(0, v)) * kXxP1 + kXxP4; }
// XXH64(p[0, n), seed 0): the 32-byte stripes serially, accumulator j on lane j; the tail and the avalanche wave-uniform
__device__ __forceinline__ uint64_t zs_xxh64(ZstdLds* L, const uint8_t* p, uint32_t n) {
    const uint32_t stripes = n >> 5;
    uint64_t h;
    if (stripes != 0u) {
        CJ_LANES(lane) {
            if (lane < 4u) {
                uint64_t acc = lane == 0u ? kXxP1 + kXxP2 : lane == 1u ? kXxP2 : lane == 2u ? 0ull : 0ull - kXxP1;
                const uint8_t* q = p + 8u * lane;
                for (uint32_t i = 0; i < stripes; i++, q += 32)
                    acc = zs_xx_round(acc, (uint64_t)out_rd32(q) | ((uint64_t)out_rd32(q + 4) << 32));
                L->acc[2u * lane] = (uint32_t)acc;
                L->acc[2u * lane + 1u] = (uint32_t)(acc >> 32);
            }
        }
        wave_order();
        uint64_t v[4];
        for (uint32_t j = 0; j < 4u; j++) v[j] = (uint64_t)lds_ld(&L->acc[2u * j]) | ((uint64_t)lds_ld(&L->acc[2u * j + 1u]) << 32);
        h = zs_rotl(v[0], 1) + zs_rotl(v[1], 7) + zs_rotl(v[2], 12) + zs_rotl(v[3], 18);
        for (uint32_t j = 0; j < 4u; j++) h = zs_xx_merge(h, v[j]);
        wave_order();
    } else {
        h = kXxP5;
    }
    h += n;
    uint32_t at = stripes << 5;
    auto le = [&](uint32_t k) { uint64_t x = 0; for (uint32_t j = 0; j < k; j++) x |= (uint64_t)out_ld8(p + at + j) << (8u * j); at += k; return x; };
    while (at + 8u <= n) { h ^= zs_xx_round(0, le(8)); h = zs_rotl(h, 27) * kXxP1 + kXxP4; }
    if (at + 4u <= n) { h ^= le(4) * kXxP1; h = zs_rotl(h, 23) * kXxP2 + kXxP3; }
    while (at < n) { h ^= le(1) * kXxP5; h = zs_rotl(h, 11) * kXxP1; }
    h ^= h >> 33; h *= kXxP2; h ^= h >> 29; h *= kXxP3; h ^= h >> 32;
    return h;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
// Decode one chunk (wave-uniform arguments): n <= 0x7FFFFFF0 bytes at in, cap <= 0x7E000000 bytes at out, slot: kZsSlotBytes of
// global memory that are this wavefront's own.  Returns the decoded length or CJ_E_*: libzstd's ZSTD_decompress(out, cap, in, n).
// SIZE: the size query (top of the file); out, cap and slot are not used, a total above 0x7E000000 is CJ_E_PREFIX_TOO_BIG.
template <bool SIZE>
__device__ __forceinline__ int64_t zstd_wave_decode(const uint8_t* in_ptr, uint32_t n, uint8_t* out, uint32_t cap, ZstdLds* L, uint8_t* slot) {
    const uint32_t room = SIZE ? kZsOutMax : cap;
    const int64_t full = SIZE ? CJ_E_PREFIX_TOO_BIG : CJ_E_OUT_TOO_SMALL;
    ZsIn in;
    in.init(in_ptr, n);
    uint32_t ip = in.w.iend - n;                   // positions relative to in.w.base
    const uint32_t iend = in.w.iend;
    uint32_t op = 0;
    bool more_than_one = false;

    while (iend - ip >= 5u) {                                                // ZSTD_decompressMultiFrame
        const uint32_t magic = in.fle(ip, 4);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {                          // a skippable frame
            if (iend - ip < 8u) return CJ_E_ZSTD_SRC_SIZE;
            const uint32_t sz = in.fle(ip + 4u, 4);
            if (sz + 8u < sz) return CJ_E_ZSTD_HEADER;
            if (sz + 8u > iend - ip) return CJ_E_ZSTD_SRC_SIZE;
            ip += sz + 8u;
            continue;
        }
        // ---- the frame header (ZSTD_decompressFrame, ZSTD_getFrameHeader) -----------------------------------------------------------
        if (iend - ip < 9u) return CJ_E_ZSTD_SRC_SIZE;
        const uint32_t fhd = in.f8(ip + 4u);
        const uint32_t single = (fhd >> 5) & 1u, did_code = fhd & 3u, fcs_code = fhd >> 6;
        const uint32_t did_len = did_code == 3u ? 4u : did_code, fcs_len = fcs_code == 0u ? single : 1u << fcs_code;
        const uint32_t fhs = 5u + (single ? 0u : 1u) + did_len + fcs_len;
        if (iend - ip < fhs + 3u) return CJ_E_ZSTD_SRC_SIZE;
        if (magic != 0xFD2FB528u) return more_than_one ? CJ_E_ZSTD_SRC_SIZE : CJ_E_ZSTD_HEADER;
        if (fhd & 8u) return CJ_E_ZSTD_HEADER;
        uint32_t q = ip + 5u;
        uint64_t window = 0;
        if (!single) {
            const uint32_t wd = in.f8(q), wlog = (wd >> 3) + 10u;
            if (wlog > 31u) return CJ_E_ZSTD_HEADER;
            window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7u);
            q += 1u;
        }
        const uint32_t did = did_len ? in.fle(q, did_len) : 0u;
        q += did_len;
        bool has_fcs = fcs_len != 0u;
        uint64_t fcs = 0;
        if (has_fcs) {
            fcs = in.fle(q, fcs_len < 4u ? fcs_len : 4u);
            if (fcs_len == 8u) fcs |= (uint64_t)in.fle(q + 4u, 4) << 32;
            if (fcs_len == 2u) fcs += 256u;
        }
        if (did != 0u) return CJ_E_ZSTD_DICT;
        if (single) window = fcs;
        const bool long_window = window > (1ull << 24);                      // libzstd considers its other sequence decoder (below)
        const bool has_sum = (fhd & 4u) != 0u;
        ip += fhs;

        // ---- the frame's state: what Repeat, Treeless and the repeat offsets carry from block to block ------------------------------
        const uint32_t fstart = op;
        uint32_t rep1 = 1, rep2 = 4, rep3 = 8;
        bool fse_valid = false, huf_valid = false, huf_x2 = false;
        uint32_t hlog = 0, ll_log = 0, of_log = 0, ml_log = 0;
        uint32_t last_block = 0;
        do {
            if (iend - ip < 3u) return CJ_E_ZSTD_SRC_SIZE;
            const uint32_t bh = in.fle(ip, 3);
            last_block = bh & 1u;
            const uint32_t btype = (bh >> 1) & 3u, bsize = bh >> 3;
            if (btype == 3u) return CJ_E_ZSTD_CORRUPT;
            const uint32_t csize = btype == 1u ? 1u : bsize;
            ip += 3u;
            if (csize > iend - ip) return CJ_E_ZSTD_SRC_SIZE;
            if (btype == 2u && csize >= kZsBlockMax) return CJ_E_ZSTD_SRC_SIZE;
            const uint32_t bend = ip + csize;
            if (SIZE && has_fcs) { ip = bend; continue; }                    // the size is the header's
            if (btype == 0u) {
                if (bsize > room - op) return full;
                if (!SIZE) { wave_order(); wave_copy(out + op, in.w.base + ip, bsize); wave_order(); }
                op += bsize;
                ip = bend;
                continue;
            }
            if (btype == 1u) {
                if (bsize > room - op) return full;
                if (!SIZE && bsize != 0u) {
                    LaneBytes b;
                    b.put(0u, in.f8(ip));
                    wave_order();
                    b.flush(out + op, 1u);
                    wave_order();
                    wave_match_copy(out + op + 1u, 1u, bsize - 1u);
                    wave_order();
                }
                op += bsize;
                ip = bend;
                continue;
            }
            // ---- a compressed block: the literals section (ZSTD_decodeLiteralsBlock) ----------------------------------------------------
            if (csize < 3u) return CJ_E_ZSTD_CORRUPT;
            const uint32_t b0 = in.f8(ip), lkind = b0 & 3u, lhl = (b0 >> 2) & 3u;
            uint32_t lit_size, lit_kind, lit_src = 0, lit_byte = 0;          // lit_kind 0: in the input at lit_src; 1: lit_byte repeated; 2: in the slot
            if (lkind >= 2u) {
                if (lkind == 3u && !SIZE && !huf_valid) return CJ_E_ZSTD_CORRUPT;      // (libzstd: dictionary_corrupted)
                if (csize < 5u) return CJ_E_ZSTD_CORRUPT;
                const uint32_t lhc = in.fle(ip, 4);
                uint32_t lh, lcs;
                const bool one = lhl == 0u;
                if (lhl < 2u) { lh = 3u; lit_size = (lhc >> 4) & 0x3FFu; lcs = (lhc >> 14) & 0x3FFu; }
                else if (lhl == 2u) { lh = 4u; lit_size = (lhc >> 4) & 0x3FFFu; lcs = lhc >> 18; }
                else { lh = 5u; lit_size = (lhc >> 4) & 0x3FFFFu; lcs = (lhc >> 22) + (in.f8(ip + 4u) << 10); }
                if (lit_size > kZsBlockMax) return CJ_E_ZSTD_CORRUPT;
                if (lcs + lh > csize) return CJ_E_ZSTD_CORRUPT;
                lit_kind = 2u;
                if (!SIZE) {
                    uint32_t hpos = ip + lh, hsize = lcs;
                    if (lkind == 2u) {
                        const uint32_t h = zs_huf_read(in, L, hpos, hsize, hlog);
                        if (h == 0u || h >= hsize) return CJ_E_ZSTD_CORRUPT;
                        hpos += h; hsize -= h;
                        huf_x2 = !one && zs_huf_select_x2(lit_size, lcs);
                    }
                    uint32_t l1 = hsize, l2 = 0, l3 = 0, seg = lit_size;
                    if (!one) {
                        if (lkind == 2u && lit_size == 0u) return CJ_E_ZSTD_CORRUPT;
                        if (hsize < 10u) return CJ_E_ZSTD_CORRUPT;
                        l1 = in.fle(hpos, 2); l2 = in.fle(hpos + 2u, 2); l3 = in.fle(hpos + 4u, 2);
                        if (l1 + l2 + l3 + 6u > hsize) return CJ_E_ZSTD_CORRUPT;
                        seg = (lit_size + 3u) / 4u;
                        hpos += 6u;
                    }
                    const uint32_t l4 = one ? 0u : hsize - 6u - l1 - l2 - l3, n4 = lit_size > 3u * seg ? lit_size - 3u * seg : 0u;
                    const uint8_t* hsrc = in.w.base + hpos;
                    const uint32_t log = hlog;
                    const bool x2 = huf_x2;
                    CJ_LANES(lane) { if (lane == 0u) L->flag = 0u; }
                    wave_order();
                    CJ_LANES(lane) {
                        if (lane < (one ? 1u : 4u)) {
                            const uint32_t soff = lane == 0u ? 0u : lane == 1u ? l1 : lane == 2u ? l1 + l2 : l1 + l2 + l3;
                            const uint32_t slen = lane == 0u ? l1 : lane == 1u ? l2 : lane == 2u ? l3 : l4;
                            const uint32_t scount = one ? lit_size : lane == 3u ? n4 : seg;
                            const bool ok = x2 ? zs_huf_stream_x2(L, log, hsrc + soff, slen, slot + lane * seg, scount)
                                               : zs_huf_stream(L, log, hsrc + soff, slen, slot + lane * seg, scount);
                            if (!ok) lds_or(&L->flag, 1u);
                        }
                    }
                    wave_order();
                    if (lds_ld(&L->flag) != 0u) return CJ_E_ZSTD_CORRUPT;
                    huf_valid = true;
                }
                ip += lh + lcs;
            } else {
                uint32_t lh;
                if (lhl == 0u || lhl == 2u) { lh = 1u; lit_size = b0 >> 3; }
                else if (lhl == 1u) { lh = 2u; lit_size = in.fle(ip, 2) >> 4; }
                else {
                    lh = 3u; lit_size = in.fle(ip, 3) >> 4;
                    if (lkind == 1u && csize < 4u) return CJ_E_ZSTD_CORRUPT;
                }
                if (lkind == 0u) {
                    if (lh + lit_size > csize) return CJ_E_ZSTD_CORRUPT;
                    lit_kind = 0u; lit_src = ip + lh;
                    ip += lh + lit_size;
                } else {
                    if (lit_size > kZsBlockMax) return CJ_E_ZSTD_CORRUPT;
                    lit_kind = 1u; lit_byte = in.f8(ip + lh);
                    ip += lh + 1u;
                }
            }
            uint32_t lit_pos = 0;
            // `k` literals of the block to out + op (the caller has checked the room and the count)
            auto put_literals = [&](uint32_t k) {
                if (SIZE || k == 0u) return;
                wave_order();
                if (lit_kind == 0u) wave_copy(out + op, in.w.base + lit_src + lit_pos, k);
                else if (lit_kind == 2u) wave_copy(out + op, slot + lit_pos, k);
                else {
                    LaneBytes b;
                    b.put(0u, lit_byte);
                    wave_order();
                    b.flush(out + op, 1u);
                    wave_order();
                    wave_match_copy(out + op + 1u, 1u, k - 1u);
                }
                wave_order();
            };

            // ---- the sequences section (ZSTD_decodeSeqHeaders, ZSTD_decompressSequences) ------------------------------------------------
            if (ip >= bend) return CJ_E_ZSTD_SRC_SIZE;
            uint32_t nseq = in.f8(ip++);
            if (nseq == 0u) {
                if (ip != bend) return CJ_E_ZSTD_SRC_SIZE;
            } else {
                if (nseq > 0x7Fu) {
                    if (nseq == 0xFFu) {
                        if (ip + 2u > bend) return CJ_E_ZSTD_SRC_SIZE;
                        nseq = in.fle(ip, 2) + 0x7F00u;
                        ip += 2u;
                    } else {
                        if (ip >= bend) return CJ_E_ZSTD_SRC_SIZE;
                        nseq = ((nseq - 0x80u) << 8) + in.f8(ip++);
                    }
                }
                if (ip + 1u > bend) return CJ_E_ZSTD_SRC_SIZE;
                const uint32_t modes = in.f8(ip++);
                if (!zs_seq_table(in, L, 0u, modes >> 6, ip, bend, fse_valid, ll_log)) return CJ_E_ZSTD_CORRUPT;
                if (!zs_seq_table(in, L, 1u, (modes >> 4) & 3u, ip, bend, fse_valid, of_log)) return CJ_E_ZSTD_CORRUPT;
                if (!zs_seq_table(in, L, 2u, (modes >> 2) & 3u, ip, bend, fse_valid, ml_log)) return CJ_E_ZSTD_CORRUPT;
            }
            if (nseq != 0u) {
                fse_valid = true;
                ZsBitD b;
                if (!b.init(in, ip, bend - ip)) return CJ_E_ZSTD_CORRUPT;
                uint32_t st_ll = b.read(ll_log); b.reload(in);
                uint32_t st_of = b.read(of_log); b.reload(in);
                uint32_t st_ml = b.read(ml_log); b.reload(in);
                // libzstd has a second sequence decoder, which decodes four sequences ahead of the one it executes
                // (ZSTD_decompressSequencesLong), and takes it in a frame whose window is above 16 MiB for a block of more than 4
                // sequences whose offset table has 7 of 256 cells or more with over 22 extra bits.  It reads the same sequences but
                // ends differently: it looks for an over-read BEFORE it decodes a sequence, and refuses then, four sequences short
                // of that one executed; and it does not ask whether bits are left at the end.
                uint32_t todo = nseq;
                bool prefetch = false, cut = false;
                if (long_window && nseq > 4u) {
                    uint32_t share = 0;
                    for (uint32_t u = 0; u < (1u << of_log); u++) share += (lds_ld(&L->fse[kZsOF + u]) & 255u) > 22u ? 1u : 0u;
                    prefetch = (share << (8u - of_log)) >= 7u;
                }
                if (prefetch) {                                              // how far that decoder gets: the same walk without the sequences' values
                    ZsBitD pb = b;
                    uint32_t p_ll = st_ll, p_of = st_of, p_ml = st_ml, k = 0;
                    for (; k < nseq; k++) {
                        if (pb.reload(in) == kZsOverflow) break;
                        const uint32_t e_ll = lds_ld(&L->fse[kZsLL + (p_ll & 511u)]), e_ml = lds_ld(&L->fse[kZsML + (p_ml & 511u)]);
                        const uint32_t e_of = lds_ld(&L->fse[kZsOF + (p_of & 255u)]);
                        uint32_t base, ll_bits, ml_bits;
                        zs_ll_code(e_ll & 255u, base, ll_bits);
                        zs_ml_code(e_ml & 255u, base, ml_bits);
                        const uint32_t of_bits = e_of & 255u & 31u;
                        pb.bc += of_bits + ml_bits;
                        if (ll_bits + ml_bits + of_bits >= 31u) pb.reload(in);
                        pb.bc += ll_bits;
                        p_ll = (e_ll >> 16) + pb.read((e_ll >> 8) & 255u);
                        p_ml = (e_ml >> 16) + pb.read((e_ml >> 8) & 255u);
                        p_of = (e_of >> 16) + pb.read((e_of >> 8) & 255u);
                    }
                    if (k < nseq) {
                        if (k <= 4u) return CJ_E_ZSTD_CORRUPT;               // found before anything was executed
                        cut = true;                                          // ... behind sequences 0 .. k - 5: their errors come first
                        todo = k - 4u;
                    }
                }
                uint32_t r1 = rep1, r2 = rep2, r3 = rep3;
                for (;;) {                                                   // todo turns
                    const uint32_t e_ll = lds_ld(&L->fse[kZsLL + (st_ll & 511u)]), e_ml = lds_ld(&L->fse[kZsML + (st_ml & 511u)]);
                    const uint32_t e_of = lds_ld(&L->fse[kZsOF + (st_of & 255u)]);
                    uint32_t ll, ll_bits, ml, ml_bits;
                    zs_ll_code(e_ll & 255u, ll, ll_bits);
                    zs_ml_code(e_ml & 255u, ml, ml_bits);
                    const uint32_t of_bits = e_of & 255u & 31u;
                    const uint32_t ll0 = (e_ll & 255u) == 0u ? 1u : 0u;
                    uint32_t offset;
                    if (of_bits > 1u) {
                        offset = ((1u << of_bits) - 3u) + b.read_fast(of_bits);
                        r3 = r2; r2 = r1; r1 = offset;
                    } else if (of_bits == 0u) {
                        if (!ll0) offset = r1;
                        else { offset = r2; r2 = r1; r1 = offset; }
                    } else {
                        const uint32_t idx = 1u + ll0 + b.read_fast(1u);
                        uint32_t t = idx == 3u ? r1 - 1u : idx == 1u ? r2 : r3;
                        if (t == 0u) t = 1u;
                        if (idx != 1u) r3 = r2;
                        r2 = r1;
                        r1 = offset = t;
                    }
                    if (ml_bits != 0u) ml += b.read_fast(ml_bits);
                    if (ll_bits + ml_bits + of_bits >= 31u) b.reload(in);
                    if (ll_bits != 0u) ll += b.read_fast(ll_bits);
                    st_ll = (e_ll >> 16) + b.read((e_ll >> 8) & 255u);
                    st_ml = (e_ml >> 16) + b.read((e_ml >> 8) & 255u);
                    st_of = (e_of >> 16) + b.read((e_of >> 8) & 255u);
                    // ZSTD_execSequence: the room, the literals, the offset — in that order
                    if ((uint64_t)ll + ml > (uint64_t)(room - op)) return full;
                    if (ll > lit_size - lit_pos) return CJ_E_ZSTD_CORRUPT;
                    put_literals(ll);
                    op += ll; lit_pos += ll;
                    if (offset > op - fstart) return CJ_E_ZSTD_CORRUPT;
                    if (!SIZE) { wave_match_copy(out + op, offset, ml); wave_order(); }
                    op += ml;
                    if (--todo == 0u) break;
                    b.reload(in);
                }
                if (cut || (!prefetch && b.reload(in) < kZsCompleted)) return CJ_E_ZSTD_CORRUPT;
                rep1 = r1; rep2 = r2; rep3 = r3;
            }
            const uint32_t rest = lit_size - lit_pos;
            if (rest > room - op) return full;
            put_literals(rest);
            op += rest;
            ip = bend;
        } while (!last_block);

        // ---- the end of the frame -------------------------------------------------------------------------------------------------
        if (SIZE && has_fcs) {
            if (fcs > (uint64_t)(room - op)) return full;
            op += (uint32_t)fcs;
        } else if (has_fcs && fcs != (uint64_t)(op - fstart)) return CJ_E_ZSTD_CORRUPT;
        if (has_sum) {
            if (iend - ip < 4u) return CJ_E_ZSTD_CHECKSUM;
            if (!SIZE) {
                wave_order();
                const uint64_t h = zs_xxh64(L, out + fstart, op - fstart);
                if (in.fle(ip, 4) != (uint32_t)h) return CJ_E_ZSTD_CHECKSUM;
            }
            ip += 4u;
        }
        more_than_one = true;
    }
    if (ip != iend) return CJ_E_ZSTD_SRC_SIZE;
    return (int64_t)op;
}

}  // namespace cj
