// deflate_enc_wave.hpp compiled for the host: the kernel's own entropy stage with stand-ins for the lanes, LDS, the scratch slot and the
// output, for tests/test_deflate_encode_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases: the form a
// sanitizer build takes).  The matcher is the model's (deflate_enc_model.c: dfe_model_records, linked in) — on the device it is
// enc2::Walk<DeflateFmt, 2>, held to the same records by the GPU tests.  The stand-ins abort on any read outside the piece, any store
// outside the capacity, any record outside the slot and any LDS access through an accessor outside the wavefront's DfeLds; the LDS
// block, the slot and (SIM_MAIN) the buffers are heap blocks of exactly their size.  A CJ_LANES body runs for lanes 0..63 one after
// another: the header's rule (no body reads what another lane wrote in the same body) is what makes that the wavefront's result.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/cramjam_hip.h"
#define __device__
#define __host__
#define __forceinline__ inline
#define CJ_LANES(lane) for (uint32_t lane = 0; lane < 64u; lane++)

extern "C" uint32_t dfe_model_records(const uint8_t* in, uint32_t n, uint32_t* rec);

namespace cj {

static const uint8_t *g_in, *g_in_end;
static uint8_t *g_out, *g_out_end;
static const uint8_t *g_lds, *g_lds_end;
static const uint8_t *g_slot, *g_slot_end;

struct LaneU32 { uint32_t v[64]; uint32_t& operator[](uint32_t l) { if (l >= 64u) abort(); return v[l]; } };
struct LaneU64 { uint64_t v[64]; uint64_t& operator[](uint32_t l) { if (l >= 64u) abort(); return v[l]; } };
static uint32_t lane_excl_add(LaneU32& x, LaneU32& before) {
    uint32_t run = 0;
    for (uint32_t l = 0; l < 64u; l++) { before.v[l] = run; run += x.v[l]; }
    return run;
}
static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    if (n && (src < g_in || src + n > g_in_end || dst < g_out || dst + n > g_out_end)) abort();
    memcpy(dst, src, n);
}
static void wave_order() {}
static void lds_check(const void* p, size_t n) {
    if ((const uint8_t*)p < g_lds || (const uint8_t*)p + n > g_lds_end) abort();
}
static uint32_t lds_ld(const uint32_t* p) { lds_check(p, 4); return *p; }
static uint32_t lds_ld8(const uint8_t* p) { lds_check(p, 1); return *p; }
static void lds_add(uint32_t* p, uint32_t v) { lds_check(p, 4); *p += v; }
static void lds_or(uint32_t* p, uint32_t v) { lds_check(p, 4); *p |= v; }
static uint32_t in_ld8(const uint8_t* p) { if (p < g_in || p >= g_in_end) abort(); return *p; }
static void out_st32(uint8_t* p, uint32_t v) { if (p < g_out || p + 4 > g_out_end) abort(); memcpy(p, &v, 4); }
static void out_st8(uint8_t* p, uint32_t v) { if (p < g_out || p >= g_out_end) abort(); *p = (uint8_t)v; }
struct DfeRec;
static DfeRec rec_ld(const DfeRec* slot, uint32_t i);

}  // namespace cj

#include "../../cramjam_amd/csrc/deflate_enc_wave.hpp"
#include "../../cramjam_amd/csrc/crc32_lanes.hpp"

namespace cj {
static DfeRec rec_ld(const DfeRec* slot, uint32_t i) {
    if ((const uint8_t*)(slot + i) < g_slot || (const uint8_t*)(slot + i + 1) > g_slot_end) abort();
    return slot[i];
}
}

static cj::DfeLds* new_lds() {
    cj::DfeLds* L = (cj::DfeLds*)malloc(sizeof(cj::DfeLds));
    memset(L, 0xA5, sizeof *L);                      // LDS holds whatever ran before
    cj::g_lds = (const uint8_t*)L; cj::g_lds_end = cj::g_lds + sizeof *L;
    return L;
}

static uint32_t adler32_of(const uint8_t* p, uint64_t n) {
    uint32_t a = 1, b = 0;
    for (uint64_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
static uint32_t crc32_of(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? cj::kCrc32Poly : 0u); }
    return ~c;
}

// One stream, as the kernel's first wavefront walks it.  types (may be null): the block type of every piece
extern "C" long long sim_deflate_encode(int wrap, const unsigned char* in, unsigned long long n, unsigned char* out, unsigned long long cap64, unsigned char* types) {
    if (n > cj::kDfeInMax) return CJ_E_INPUT_TOO_LARGE;
    cj::DfeLds* L = new_lds();
    const uint32_t cap = (uint32_t)(cap64 < 0xFFFFFFF0ull ? cap64 : 0xFFFFFFF0ull);
    cj::g_out = out; cj::g_out_end = out + cap;
    cj::DfeOut W;
    long long r = CJ_E_OUT_TOO_SMALL;
    bool ok = cj::dfe_begin(L, W, wrap, out, cap);
    const uint64_t np = n == 0 ? 1 : (n + cj::kDfePiece - 1) / cj::kDfePiece;
    for (uint64_t p = 0; p < np && ok; p++) {
        const uint8_t* pin = in + p * cj::kDfePiece;
        const uint32_t pn = (uint32_t)(n - p * cj::kDfePiece < cj::kDfePiece ? n - p * cj::kDfePiece : cj::kDfePiece);
        cj::DfeRec* slot = (cj::DfeRec*)malloc(sizeof(cj::DfeRec) * (pn / 4u + 2u));      // exactly what this piece may need
        const uint32_t nrec = dfe_model_records(pin, pn, (uint32_t*)slot);
        cj::g_in = pin; cj::g_in_end = pin + pn;
        cj::g_slot = (const uint8_t*)slot; cj::g_slot_end = (const uint8_t*)(slot + nrec);
        uint32_t t = 0;
        ok = cj::dfe_piece(L, W, pin, pn, slot, nrec, p + 1 == np, cj::dfe_tail_bytes(wrap), &t);
        if (types) types[p] = (unsigned char)t;
        free(slot);
    }
    if (ok) r = cj::dfe_end(L, W, wrap, wrap == cj::kDfeZlib ? adler32_of(in, n) : wrap == cj::kDfeGzip ? crc32_of(in, n) : 0u, (uint32_t)n);
    free(L);
    return r;
}

// the code builder alone: lens[0, nsym) from hist[0, nsym)
extern "C" void sim_dfe_build_lens(const unsigned int* hist, unsigned int nsym, unsigned int maxbits, int pad_single, unsigned char* lens) {
    cj::DfeLds* L = new_lds();
    for (uint32_t s = 0; s < nsym && s < 288u; s++) L->hist[s] = hist[s];
    cj::dfe_build_lens(L, L->hist, nsym, maxbits, pad_single != 0, L->lens);
    memcpy(lens, L->lens, nsym);
    free(L);
}
// ... and the canonical codes of given lengths: code[s] = bit-reversed code | length << 16
extern "C" void sim_dfe_assign_codes(const unsigned char* lens, unsigned int nsym, unsigned int maxbits, unsigned int* code) {
    cj::DfeLds* L = new_lds();
    memcpy(L->lens, lens, nsym);
    cj::dfe_assign_codes(L, L->lens, nsym, maxbits, L->code);
    memcpy(code, L->code, 4u * nsym);
    free(L);
}
extern "C" unsigned long long sim_dfe_bound(unsigned long long n, int wrap) { return cj::dfe_bound(n, wrap); }

#ifdef SIM_MAIN
// cases file: u32 count, then per case u32 wrap, n, cap, in_mis, out_mis | i64 expected result | input | expected stream (result > 0).
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
        const uint32_t wrap = h[0], n = h[1], cap = h[2], mi = h[3], mo = h[4];
        const size_t nexp = want > 0 ? (size_t)want : 0;
        uint8_t* in = (uint8_t*)malloc(n + mi ? n + mi : 1); uint8_t* out = (uint8_t*)malloc(cap + mo ? cap + mo : 1); uint8_t* exp = (uint8_t*)malloc(nexp ? nexp : 1);
        if ((n && fread(in + mi, 1, n, f) != n) || (nexp && fread(exp, 1, nexp, f) != nexp)) return 2;
        const long long r = sim_deflate_encode((int)wrap, in + mi, n, out + mo, cap, nullptr);
        if (r != want || (nexp && memcmp(out + mo, exp, nexp) != 0)) { bad++; printf("case %u: got %lld want %lld\n", c, r, (long long)want); }
        free(in); free(out); free(exp);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
