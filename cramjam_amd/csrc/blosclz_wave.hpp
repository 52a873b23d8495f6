// blosclz_wave.hpp — the BloscLZ stream decoder of one wavefront (blosclz_decode.hip says what the format is).  It names only
// InWindow, wave_copy, wave_match_copy and wave_order of the wave-decoder contract: wave_lanes.hpp + cj_common.hpp implement it for the device,
// tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host (sim_blosclz_decode.cpp), where
// the CPU tests hold the grammar and every copy's bounds to tests/blosclz_model.py.  Not part of the C-ABI.
#pragma once
#include "wave_window.hpp"

namespace cj {

// Decode one stream (wave-uniform arguments): the decoded size (== cap) or CJ_E_CORRUPT.  n, cap <= 0x7FFFFFF0.
__device__ __forceinline__ int64_t blosclz_wave_decode(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap) {
    if (n == 0) return CJ_E_CORRUPT;

    InWindow w;
    const uint32_t mis = window_open(w, in, n);
    const uint32_t iend = w.iend;
    uint32_t ip = mis;      // input position relative to w.base: at the top of the loop it names a control byte, ip < iend
    uint32_t op = 0;        // output position
    uint32_t mask = 31u;    // the first control byte only
    bool bad = false;

    for (;;) {
        w.ensure(ip);
        uint32_t t4 = w.fetch32(ip);
        const uint32_t ctrl = t4 & mask;
        mask = 0xffu;
        ip += 1;
        if (ctrl < 32u) {
            const uint32_t run = ctrl + 1u;
            if (run > cap - op || run > iend - ip) { bad = true; break; }
            wave_copy(out + op, w.base + ip, run);
            ip += run; op += run;
            if (ip >= iend) break;
            continue;
        }
        uint64_t len = (ctrl >> 5) - 1u;
        const uint32_t ofs = (ctrl & 31u) << 8;
        if (len == 6u) {
            uint32_t code;
            do {
                if (ip + 1u >= iend) { bad = true; break; }
                code = w.fetch32_any(ip) & 0xffu;
                ip += 1; len += code;
            } while (code == 255u);
            if (bad) break;
            t4 = w.fetch32_any(ip);                 // code and what may follow it (ip < iend: checked before the last extension byte)
        } else {
            if (ip + 1u >= iend) { bad = true; break; }
            t4 >>= 8;
        }
        const uint32_t code = t4 & 0xffu;
        ip += 1; len += 3u;
        uint32_t dist = ofs + code;
        if (code == 255u && ofs == (31u << 8)) {
            if (ip + 1u >= iend) { bad = true; break; }
            dist = (((t4 >> 8) & 0xffu) << 8) + ((t4 >> 16) & 0xffu) + 8191u;
            ip += 2;
        }
        dist += 1u;
        if (len > (uint64_t)(cap - op) || dist > op) { bad = true; break; }
        wave_order();
        wave_match_copy(out + op, dist, (uint32_t)len);
        wave_order();
        op += (uint32_t)len;
        if (ip >= iend) break;
    }
    return (bad || op != cap) ? (int64_t)CJ_E_CORRUPT : (int64_t)op;
}

}  // namespace cj
