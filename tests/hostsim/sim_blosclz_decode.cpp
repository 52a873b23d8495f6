// blosclz_wave.hpp compiled for the host: the kernel's own stream decoder with stand-ins for the wavefront's window and copies, for
// tests/test_blosclz_model.py.  The stand-ins move the same bytes and abort on any read outside the stream or write outside the
// capacity; bytes that the window would load from beyond the stream read as 0xEE, so that a decision taken on them shows.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/cramjam_hip.h"
#define __device__
#define __forceinline__ inline

namespace cj {

static const uint8_t *g_in, *g_in_end;
static uint8_t *g_out, *g_out_end;

struct InWindow {
    const uint8_t* base;
    uint32_t iend, wpos;
    void anchor(uint32_t pos) { wpos = pos & ~3u; }
    void ensure(uint32_t pos) {
        const uint32_t q = pos - wpos;
        if (q >= 256u) { if (q < 504u) wpos += 256u; else anchor(pos); }
    }
    uint32_t fetch32(uint32_t pos) const {
        if (pos - wpos > 507u) abort();                              // the register window's precondition
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(base + pos + k >= g_in && pos + k < iend ? base[pos + k] : 0xEE) << (8 * k);
        return v;
    }
    uint32_t fetch32_any(uint32_t pos) { if (pos - wpos > 500u) anchor(pos); return fetch32(pos); }
};

static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    if (n && (src < g_in || src + n > g_in_end || dst < g_out || dst + n > g_out_end)) abort();
    memcpy(dst, src, n);
}
static void wave_match_copy(uint8_t* dst, uint32_t d, uint32_t m) {
    if (d == 0 || dst - d < g_out || dst + m > g_out_end) abort();
    for (uint32_t j = 0; j < m; j++) dst[j] = dst[(int64_t)j - d];
}
static void wave_order() {}

}  // namespace cj

#include "../../cramjam_amd/csrc/blosclz_wave.hpp"

extern "C" long long sim_blosclz_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::g_in = in; cj::g_in_end = in + n; cj::g_out = out; cj::g_out_end = out + cap;
    return cj::blosclz_wave_decode(in, n, out, cap);
}
