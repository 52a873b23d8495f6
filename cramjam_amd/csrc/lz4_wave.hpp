// lz4_wave.hpp — the LZ4 block decoder of one wavefront: the sequence grammar parsed wave-uniformly out of the 512-byte register window,
// the lanes only move bytes.  Accept / reject rules of the liblz4 1.10.0 safe decoder (end-of-block parsing restrictions relative to the
// decode capacity, variable-length field limits); offset 0 is refused.  One text for the three kernels that run it:
//   kDict = false   lz4_decode_kernel (hist = 0: an independent block) and lz4_frame_chain_kernel (hist = the valid output directly in
//                   front of `out` that matches may reach: a linked LZ4-frame block), lz4_decode.hip
//   kDict = true    lz4_dict_decode_kernel (lz4_dict.hip): a block written against a DICTIONARY (LZ4_loadDict + LZ4_compress_fast_continue;
//                   read by LZ4_decompress_safe_usingDict) that does NOT lie in front of the output — only the match differs
// It names only InWindow, wave_copy, wave_match_copy and wave_order of the wave-decoder contract: wave_lanes.hpp +
// cj_common.hpp implement it for the device, tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host
// (sim_lz4_wave.cpp), where the CPU tests hold the grammar and every copy's bounds to the oracle and to tests/lz4_dict_model.py.
// Not part of the C-ABI.
#pragma once
#include "wave_window.hpp"

namespace cj {

// Decode one block (wave-uniform arguments).  hist <= 65536: the bytes that matches may reach below the block's start — kDict: the
// bytes before dict_end, the byte behind the dictionary's last one (min(dictionary length, 64 KiB): only the tail of a longer
// dictionary counts, as in liblz4); else the bytes before `out` (0, or min(position, 64 KiB) in a linked frame), dict_end unused.
// Returns the decoded size or CJ_E_CORRUPT.  n <= 0x7FFFFFF0, cap <= 0x7E000000.
template <bool kDict>
__device__ __forceinline__ int64_t lz4_wave_decode(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, const uint8_t* dict_end, uint32_t hist) {
    if (cap == 0) return (n == 1 && in[0] == 0) ? 0 : (int64_t)CJ_E_CORRUPT;
    if (n == 0) return CJ_E_CORRUPT;

    InWindow w;
    const uint32_t mis = window_open(w, in, n);
    const uint32_t iend = w.iend;
    uint32_t ip = mis;      // input position relative to w.base
    uint32_t op = 0;        // output position
    bool bad = false;

    for (;;) {
        w.ensure(ip);
        const uint32_t t4 = w.fetch32(ip);
        const uint32_t token = t4 & 0xffu;
        ip += 1;
        uint64_t lit = token >> 4;
        if (lit == 15u) {
            // variable-length literal count: bytes may not reach into the last 15 input bytes
            if (ip + 15u >= iend) { bad = true; break; }
            uint32_t b = (t4 >> 8) & 0xffu;
            ip += 1; lit += b;
            if (ip + 15u > iend) { bad = true; break; }
            while (b == 255u) {
                b = w.fetch32_any(ip) & 0xffu;
                ip += 1; lit += b;
                if (ip + 15u > iend) { bad = true; break; }
            }
            if (bad) break;
        }
        const uint32_t rem_out = cap - op, rem_in = iend - ip;
        if ((uint64_t)rem_out < lit + 12u || (uint64_t)rem_in < lit + 8u) {
            // must be the final sequence: consumes the input exactly, fits the output
            if (rem_in != lit || rem_out < lit) { bad = true; break; }
            wave_copy(out + op, w.base + ip, (uint32_t)lit);
            op += (uint32_t)lit;
            break;
        }
        wave_copy(out + op, w.base + ip, (uint32_t)lit);
        ip += (uint32_t)lit; op += (uint32_t)lit;

        const uint32_t o4 = w.fetch32_any(ip);
        const uint32_t offset = o4 & 0xffffu;
        ip += 2;
        uint64_t mlen = token & 15u;
        if (mlen == 15u) {
            uint32_t b = (o4 >> 16) & 0xffu;
            ip += 1; mlen += b;
            if (ip + 4u > iend) { bad = true; break; }
            while (b == 255u) {
                b = w.fetch32_any(ip) & 0xffu;
                ip += 1; mlen += b;
                if (ip + 4u > iend) { bad = true; break; }
            }
            if (bad) break;
        }
        mlen += 4u;
        if (offset == 0u || (uint64_t)offset > (uint64_t)op + hist) { bad = true; break; }
        if ((uint64_t)(cap - op) < mlen + 5u) { bad = true; break; }   // last 5 bytes are literals
        // (two arms of their own: `kDict && offset > op` around a shared tail would give the plain kernels the m != 0 branch)
        if constexpr (kDict) {
            uint32_t m = (uint32_t)mlen, at = op;
            if (offset > op) {
                // the match starts `back` bytes before the dictionary's end: that part is a plain copy from the dictionary; what is left
                // of it continues at out + 0 with the same offset
                const uint32_t back = offset - op;
                const uint32_t d = m < back ? m : back;
                wave_copy(out + at, dict_end - back, d);
                at += d; m -= d;
            }
            if (m != 0u) {
                wave_order();
                wave_match_copy(out + at, offset, m);
            }
            wave_order();
        } else {
            wave_order();
            wave_match_copy(out + op, offset, (uint32_t)mlen);
            wave_order();
        }
        op += (uint32_t)mlen;
    }
    return bad ? (int64_t)CJ_E_CORRUPT : (int64_t)op;
}

}  // namespace cj
