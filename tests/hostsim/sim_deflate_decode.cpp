// deflate_wave.hpp compiled for the host: the kernel's own DEFLATE decoder with stand-ins for the wavefront's window, copies, lanes and
// LDS, for tests/test_deflate_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases: the form a sanitizer
// build takes).  The stand-ins move the same bytes and end the decode with SIM_BOUNDS (-9999, no CJ_E_* code) on any read outside the
// stream, any write outside the capacity and any LDS access outside the wavefront's DeflateLds, so that a test fails by name; bytes that the window would load from beyond the stream read as 0xEE, so that a
// decision taken on them shows.  A CJ_LANES body runs for lanes 0..63 one after another: the header's rule (no body reads what
// another lane wrote in the same body) is what makes that the wavefront's result.
#include <setjmp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/cramjam_hip.h"
#define __device__
#define __forceinline__ inline
#define CJ_LANES(lane) for (uint32_t lane = 0; lane < 64u; lane++)

namespace cj {

static const uint8_t *g_in, *g_in_end;
static uint8_t *g_out, *g_out_end;
static const uint8_t *g_lds, *g_lds_end;
static jmp_buf g_fail;                                                   // back into sim_deflate_decode (no frame between holds a destructor)
[[noreturn]] static void sim_fail() { longjmp(g_fail, 1); }

struct InWindow {
    const uint8_t* base;
    uint32_t iend, wpos;
    void anchor(uint32_t pos) { wpos = pos & ~3u; }
    void ensure(uint32_t pos) {
        const uint32_t q = pos - wpos;
        if (q >= 256u) { if (q < 504u) wpos += 256u; else anchor(pos); }
    }
    uint32_t fetch32(uint32_t pos) const {
        if (pos - wpos > 507u) sim_fail();                              // the register window's precondition
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(base + pos + k >= g_in && pos + k < iend ? base[pos + k] : 0xEE) << (8 * k);
        return v;
    }
};

static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    if (n && (src < g_in || src + n > g_in_end || dst < g_out || dst + n > g_out_end)) sim_fail();
    memcpy(dst, src, n);
}
static void wave_match_copy(uint8_t* dst, uint32_t d, uint32_t m) {
    if (d == 0 || dst - d < g_out || dst + m > g_out_end) sim_fail();
    for (uint32_t j = 0; j < m; j++) dst[j] = dst[(int64_t)j - d];
}
static void wave_order() {}

static void lds_check(const void* p, size_t n) {
    if ((const uint8_t*)p < g_lds || (const uint8_t*)p + n > g_lds_end) sim_fail();
}
static uint32_t lds_ld(const uint32_t* p) { lds_check(p, 4); return *p; }
static uint32_t lds_ld8(const uint8_t* p) { lds_check(p, 1); return *p; }
static uint32_t out_ld8(const uint8_t* p) { if (p < g_out || p >= g_out_end) sim_fail(); return *p; }
static void lds_add(uint32_t* p, uint32_t v) { lds_check(p, 4); *p += v; }
static void lds_xor(uint32_t* p, uint32_t v) { lds_check(p, 4); *p ^= v; }

struct LaneBytes {
    uint8_t v[64];
    void put(uint32_t k, uint32_t byte) { if (k >= 64u) sim_fail(); v[k] = (uint8_t)byte; }
    void flush(uint8_t* dst, uint32_t n) {
        if (n > 64u || dst < g_out || dst + n > g_out_end) sim_fail();
        memcpy(dst, v, n);
    }
};

}  // namespace cj

#include "../../cramjam_amd/csrc/deflate_wave.hpp"

static const cj::Crc32Tables g_crc = cj::make_crc32_tables();

// wrap: a cj_deflate_wrap; size != 0: the size query (out and cap are not used).  The LDS block is a heap block of exactly its size,
// filled with 0xA5 as LDS is with whatever ran before.
extern "C" long long sim_deflate_decode(int wrap, int size, const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::DeflateLds* L = (cj::DeflateLds*)malloc(sizeof(cj::DeflateLds));
    memset(L, 0xA5, sizeof *L);
    cj::g_in = in; cj::g_in_end = in + n; cj::g_out = out; cj::g_out_end = out + (size ? 0 : cap);
    cj::g_lds = (const uint8_t*)L; cj::g_lds_end = cj::g_lds + sizeof *L;
    const uint32_t* adv = &g_crc.adv256[0][0];
    if (setjmp(cj::g_fail)) { free(L); return -9999; }                   // SIM_BOUNDS: a stand-in's check fired
    long long r = CJ_E_BAD_ARG;
    if (!size) {
        if (wrap == 0) r = cj::deflate_wave_decode<0, false>(in, n, out, cap, L, adv, g_crc.xpow8);
        if (wrap == 1) r = cj::deflate_wave_decode<1, false>(in, n, out, cap, L, adv, g_crc.xpow8);
        if (wrap == 2) r = cj::deflate_wave_decode<2, false>(in, n, out, cap, L, adv, g_crc.xpow8);
    } else {
        if (wrap == 0) r = cj::deflate_wave_decode<0, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
        if (wrap == 1) r = cj::deflate_wave_decode<1, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
        if (wrap == 2) r = cj::deflate_wave_decode<2, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
    }
    free(L);
    return r;
}

#ifdef SIM_MAIN
// cases file: u32 count, then per case u32 wrap, size, n, cap, mis | i64 expected result | stream | expected bytes (decode mode, result > 0).
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
        const uint32_t wrap = h[0], size = h[1], n = h[2], cap = h[3], mi = h[4];
        const size_t nexp = (!size && want > 0) ? (size_t)want : 0;
        uint8_t* in = (uint8_t*)malloc(n + mi ? n + mi : 1); uint8_t* out = (uint8_t*)malloc(cap ? cap : 1); uint8_t* exp = (uint8_t*)malloc(nexp ? nexp : 1);
        if ((n && fread(in + mi, 1, n, f) != n) || (nexp && fread(exp, 1, nexp, f) != nexp)) return 2;
        const long long r = sim_deflate_decode((int)wrap, (int)size, in + mi, n, out, cap);
        if (r != want || (nexp && memcmp(out, exp, nexp) != 0)) { bad++; printf("case %u: got %lld want %lld\n", c, r, (long long)want); }
        free(in); free(out); free(exp);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
