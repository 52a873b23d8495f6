// zstd_wave.hpp compiled for the host: the kernel's own Zstandard decoder with stand-ins for the wavefront's window, copies, lanes, LDS
// and literal slot, for tests/test_zstd_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases: the form a
// sanitizer build takes).  The stand-ins move the same bytes and end the decode with SIM_BOUNDS (-9999, no CJ_E_* code) on any read
// outside the stream, any write outside the capacity or the slot and any LDS access outside the wavefront's ZstdLds; bytes that the
// window would load from beyond the stream read as 0xEE, so that a decision taken on them shows.  A CJ_LANES body runs for lanes
// 0..63 one after another.
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
static uint8_t *g_slot, *g_slot_end;
static const uint8_t *g_lds, *g_lds_end;
static jmp_buf g_fail;
[[noreturn]] static void sim_fail() { longjmp(g_fail, 1); }

struct InWindow {
    const uint8_t* base;
    uint32_t iend, wpos;
    void anchor(uint32_t pos) { wpos = pos & ~3u; }
    uint32_t fetch32(uint32_t pos) const {
        if (pos - wpos > 507u) sim_fail();                              // the register window's precondition
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(base + pos + k >= g_in && pos + k < iend ? base[pos + k] : 0xEE) << (8 * k);
        return v;
    }
};

static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const bool from_in = src >= g_in && src + n <= g_in_end, from_slot = src >= g_slot && src + n <= g_slot_end;
    if (n && ((!from_in && !from_slot) || dst < g_out || dst + n > g_out_end)) sim_fail();
    memcpy(dst, src, n);
}
static void wave_match_copy(uint8_t* dst, uint32_t d, uint32_t m) {
    if (m == 0) return;
    if (d == 0 || dst - d < g_out || dst + m > g_out_end) sim_fail();
    for (uint32_t j = 0; j < m; j++) dst[j] = dst[(int64_t)j - d];
}
static void wave_order() {}

static void lds_check(const void* p, size_t n) {
    if ((const uint8_t*)p < g_lds || (const uint8_t*)p + n > g_lds_end) sim_fail();
}
static uint32_t lds_ld(const uint32_t* p) { lds_check(p, 4); return *p; }
static void lds_add(uint32_t* p, uint32_t v) { lds_check(p, 4); *p += v; }
static void lds_or(uint32_t* p, uint32_t v) { lds_check(p, 4); *p |= v; }
static uint32_t in_ld8(const uint8_t* p) { if (p < g_in || p >= g_in_end) sim_fail(); return *p; }
static uint32_t in_ld32(const uint8_t* p) { if (p < g_in || p + 4 > g_in_end) sim_fail(); uint32_t v; memcpy(&v, p, 4); return v; }
static void slot_st8(uint8_t* p, uint32_t v) { if (p < g_slot || p >= g_slot_end) sim_fail(); *p = (uint8_t)v; }
static uint32_t out_ld8(const uint8_t* p) { if (p < g_out || p >= g_out_end) sim_fail(); return *p; }
static uint32_t out_rd32(const uint8_t* p) { if (p < g_out || p + 4 > g_out_end) sim_fail(); uint32_t v; memcpy(&v, p, 4); return v; }

struct LaneBytes {
    uint8_t v[64];
    void put(uint32_t k, uint32_t byte) { if (k >= 64u) sim_fail(); v[k] = (uint8_t)byte; }
    void flush(uint8_t* dst, uint32_t n) {
        if (n > 64u || dst < g_out || dst + n > g_out_end) sim_fail();
        memcpy(dst, v, n);
    }
};

}  // namespace cj

#include "../../cramjam_amd/csrc/zstd_wave.hpp"

// size != 0: the size query (out and cap are not used).  The LDS block and the slot are heap blocks of exactly their size, filled with
// 0xA5 as they are with whatever ran before.
extern "C" long long sim_zstd_decode(int size, const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::ZstdLds* L = (cj::ZstdLds*)malloc(sizeof(cj::ZstdLds));
    uint8_t* slot = (uint8_t*)malloc(cj::kZsSlotBytes);
    memset(L, 0xA5, sizeof *L);
    memset(slot, 0xA5, cj::kZsSlotBytes);
    cj::g_in = in; cj::g_in_end = in + n; cj::g_out = out; cj::g_out_end = out + (size ? 0 : cap);
    cj::g_slot = slot; cj::g_slot_end = slot + (size ? 0 : cj::kZsSlotBytes);
    cj::g_lds = (const uint8_t*)L; cj::g_lds_end = cj::g_lds + sizeof *L;
    long long r;
    if (setjmp(cj::g_fail)) r = -9999;                                   // SIM_BOUNDS: a stand-in's check fired
    else r = size ? cj::zstd_wave_decode<true>(in, n, nullptr, 0, L, nullptr) : cj::zstd_wave_decode<false>(in, n, out, cap, L, slot);
    free(L);
    free(slot);
    return r;
}

// XXH64(p[0, n), seed 0) as the lanes compute it (tests compare it with a scalar one)
extern "C" unsigned long long sim_zstd_xxh64(unsigned char* p, unsigned int n) {
    cj::ZstdLds* L = (cj::ZstdLds*)malloc(sizeof(cj::ZstdLds));
    cj::g_out = p; cj::g_out_end = p + n;
    cj::g_lds = (const uint8_t*)L; cj::g_lds_end = cj::g_lds + sizeof *L;
    unsigned long long h = 0;
    if (!setjmp(cj::g_fail)) h = cj::zs_xxh64(L, p, n);
    free(L);
    return h;
}

extern "C" unsigned int sim_zstd_lds_bytes(void) { return (unsigned int)sizeof(cj::ZstdLds); }

#ifdef SIM_MAIN
// cases file: u32 count, then per case u32 size, n, cap, mis | i64 expected result | stream | expected bytes (decode mode, result > 0).
// Every buffer is a heap block of exactly its size (plus the misalignment in front), so that a sanitizer sees each edge.
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0, bad = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        uint32_t h[4]; int64_t want;
        if (fread(h, 4, 4, f) != 4 || fread(&want, 8, 1, f) != 1) return 2;
        const uint32_t size = h[0], n = h[1], cap = h[2], mi = h[3];
        const size_t nexp = (!size && want > 0) ? (size_t)want : 0;
        uint8_t* in = (uint8_t*)malloc(n + mi ? n + mi : 1); uint8_t* out = (uint8_t*)malloc(cap ? cap : 1); uint8_t* exp = (uint8_t*)malloc(nexp ? nexp : 1);
        if ((n && fread(in + mi, 1, n, f) != n) || (nexp && fread(exp, 1, nexp, f) != nexp)) return 2;
        const long long r = sim_zstd_decode((int)size, in + mi, n, out, cap);
        if (r != want || (nexp && memcmp(out, exp, nexp) != 0)) { bad++; printf("case %u: got %lld want %lld\n", c, r, (long long)want); }
        free(in); free(out); free(exp);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
