// snappy_wave.hpp — the Snappy *raw* decoder of one wavefront (snappy_decode_kernel, snappy_decode.hip): same shape as lz4_wave.hpp, the
// tag grammar parsed wave-uniformly out of the 512-byte register window, the lanes only move bytes.  Error conditions follow snap 1.1.1
// raw::Decoder::decompress: Empty, Header (bad varint), TooBig (> u32::MAX), BufferTooSmall (preamble > capacity), and one "corrupt"
// class for Literal / CopyRead / CopyWrite / Offset / HeaderMismatch.
// It names only InWindow, wave_copy, wave_match_copy and wave_order of the wave-decoder contract: wave_lanes.hpp +
// cj_common.hpp implement it for the device, tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host
// (sim_snappy_wave.cpp), where the CPU tests hold it to the oracle on the input sweep's cases.  Not part of the C-ABI.
#pragma once
#include "wave_window.hpp"

namespace cj {

// Decode one stream (wave-uniform arguments): the decoded length, or the CJ_E_SNAPPY_* code
__device__ __forceinline__ int64_t snappy_wave_decode(const uint8_t* in, uint64_t n64, uint8_t* out, uint64_t cap64) {
    if (n64 == 0) return CJ_E_SNAPPY_EMPTY;
    if (n64 > 0xFFFFFFF0ull) return CJ_E_SNAPPY_CORRUPT;

    InWindow w;
    const uint32_t mis = window_open(w, in, (uint32_t)n64);
    const uint32_t iend = w.iend;
    uint32_t ip = mis;

    // preamble: snap bytes::read_varu64 (up to 10 bytes), then the u32 range check
    uint64_t ulen = 0;
    {
        uint32_t shift = 0, i = 0;
        bool done = false;
        while (ip < iend && i < 10u) {
            uint32_t b = w.fetch32_any(ip) & 0xffu;
            ip += 1;
            if (b < 0x80u) {
                if (i == 9u && b > 1u) break;
                ulen |= (uint64_t)b << shift;
                done = true;
                break;
            }
            ulen |= (uint64_t)(b & 0x7fu) << shift;
            shift += 7; i += 1;
        }
        if (!done) return CJ_E_SNAPPY_HEADER;
        if (ulen > 0xFFFFFFFFull) return CJ_E_SNAPPY_TOO_BIG;
        if (ulen > cap64) return CJ_E_SNAPPY_BUF_SMALL;
    }

    const uint32_t dn = (uint32_t)ulen;
    uint32_t op = 0;
    bool bad = false;

    while (ip < iend) {
        w.ensure(ip);
        const uint32_t t4 = w.fetch32(ip);
        const uint32_t tag = t4 & 0xffu;
        ip += 1;
        const uint32_t kind = tag & 3u;
        if (kind == 0u) {
            uint64_t len = (tag >> 2) + 1u;
            if (len > 60u) {
                const uint32_t nb = (uint32_t)len - 60u;        // 1..4 length bytes
                if (iend - ip < nb) { bad = true; break; }
                uint32_t v = w.fetch32_any(ip);
                if (nb < 4u) v &= (1u << (8u * nb)) - 1u;
                ip += nb;
                len = (uint64_t)v + 1u;
            }
            if (len > (uint64_t)(iend - ip) || len > (uint64_t)(dn - op)) { bad = true; break; }
            wave_copy(out + op, w.base + ip, (uint32_t)len);
            ip += (uint32_t)len; op += (uint32_t)len;
            continue;
        }
        uint32_t len, offset;
        if (kind == 1u) {
            if (iend - ip < 1u) { bad = true; break; }
            len = 4u + ((tag >> 2) & 7u);
            offset = ((tag >> 5) << 8) | ((t4 >> 8) & 0xffu);
            ip += 1;
        } else if (kind == 2u) {
            if (iend - ip < 2u) { bad = true; break; }
            len = 1u + (tag >> 2);
            offset = (t4 >> 8) & 0xffffu;
            ip += 2;
        } else {
            if (iend - ip < 4u) { bad = true; break; }
            len = 1u + (tag >> 2);
            offset = w.fetch32_any(ip);
            ip += 4;
        }
        if (offset == 0u || offset > op) { bad = true; break; }
        if (len > dn - op) { bad = true; break; }
        wave_order();
        wave_match_copy(out + op, offset, len);
        wave_order();
        op += len;
    }
    if (!bad && op != dn) bad = true;
    return bad ? (int64_t)CJ_E_SNAPPY_CORRUPT : (int64_t)dn;
}

}  // namespace cj
