// lz4_dict_wave.hpp compiled for the host: the kernel's own block decoder with stand-ins for the wavefront's window and copies, for
// tests/test_lz4_dict_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases: the form a sanitizer build takes).
// The stand-ins move the same bytes and abort on any read outside the stream or the dictionary's counted tail and on any write outside
// the capacity; bytes that the window would load from beyond the stream read as 0xEE, so that a decision taken on them shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/cramjam_hip.h"
#define __device__
#define __forceinline__ inline

namespace cj {

static const uint8_t *g_in, *g_in_end, *g_dict, *g_dict_end;
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

// literals come from the stream, the head of a match from the dictionary: nothing else is a source
static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const bool from_in = src >= g_in && src + n <= g_in_end, from_dict = src >= g_dict && src + n <= g_dict_end;
    if (n && ((!from_in && !from_dict) || dst < g_out || dst + n > g_out_end)) abort();
    memcpy(dst, src, n);
}
static void wave_match_copy(uint8_t* dst, uint32_t d, uint32_t m) {
    if (d == 0 || dst - d < g_out || dst + m > g_out_end) abort();
    for (uint32_t j = 0; j < m; j++) dst[j] = dst[(int64_t)j - d];
}
static void wave_order() {}

}  // namespace cj

#include "../../cramjam_amd/csrc/lz4_dict_wave.hpp"

// dict / dict_len: the whole dictionary; the decoder gets its end and min(dict_len, 65536), as the kernel does
extern "C" long long sim_lz4_dict_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap, const unsigned char* dict,
                                         unsigned int dict_len) {
    const unsigned int hist = dict_len < 65536u ? dict_len : 65536u;
    cj::g_in = in; cj::g_in_end = in + n; cj::g_out = out; cj::g_out_end = out + cap;
    cj::g_dict_end = dict + dict_len; cj::g_dict = cj::g_dict_end - hist;
    return cj::lz4_dict_wave_decode(in, n, out, cap, dict + dict_len, hist);
}

#ifdef SIM_MAIN
// cases file: u32 count, then per case u32 n, cap, dict_len, mis_in, mis_dict | i64 expected result | stream | dictionary | expected bytes.
// Every buffer is a heap block of exactly its size (plus the misalignment in front), so that a sanitizer sees each edge.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0, bad = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        uint32_t h[5]; int64_t want;
        if (fread(h, 4, 5, f) != 5 || fread(&want, 8, 1, f) != 1) return 2;
        const uint32_t n = h[0], cap = h[1], dl = h[2], mi = h[3], md = h[4];
        uint8_t* in = (uint8_t*)malloc(n + mi + 1); uint8_t* d = (uint8_t*)malloc(dl + md + 1); uint8_t* out = (uint8_t*)malloc(cap + 1);
        uint8_t* exp = (uint8_t*)malloc((want > 0 ? want : 0) + 1);
        if ((n && fread(in + mi, 1, n, f) != n) || (dl && fread(d + md, 1, dl, f) != dl) || (want > 0 && fread(exp, 1, want, f) != (size_t)want)) return 2;
        const long long r = sim_lz4_dict_decode(in + mi, n, out, cap, d + md, dl);
        if (r != want || (want > 0 && memcmp(out, exp, want) != 0)) { bad++; printf("case %u: got %lld want %lld\n", c, r, (long long)want); }
        free(in); free(d); free(out); free(exp);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
