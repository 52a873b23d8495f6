// sim_wave.hpp — the host implementation of the wave-decoder contract (the device's is
// cramjam_amd/csrc/wave_lanes.hpp + cj_common.hpp): what the *_wave.hpp headers name, as stand-ins that move the same bytes and check
// every access against the ranges a sim registered before it called the decoder —
//     sim_in      the stream (InWindow, in_ld8 / in_ld32, a wave_copy's source)
//     sim_out     the output up to its capacity (every copy's destination, a match's source, out_*, LaneBytes::flush)
//     sim_src2    optional, a wave_copy's other source: the dictionary's counted tail (LZ4-dict), the literal slot (zstd: slot_st8 writes it)
//     sim_lds     the wavefront's LDS block (lds_*)
//     sim_rec     the encoder's record slot (its rec_ld)
// A violation is sim_fail(): it leaves the decoder for the sim_run() that called it, which returns SIM_BOUNDS (-9999, no CJ_E_* code),
// so that a test fails by name and the process lives.  Bytes that the register window would load from beyond the stream read as 0xEE,
// so that a decision taken on them shows — or, with sim_set_device_loads(1), as the device's InWindow::load_row (cj_common.hpp) shows them:
// the memory's own bytes inside any dword that starts below iend (the up to 3 bytes below a misaligned stream and the up to 3 behind
// its end are its neighbours'), 0 in every dword behind.  The caller then owns those bytes (tests/test_neighbours_model.py).
// sim_new_block() gives LDS and slots as heap blocks of exactly their size filled with 0xA5, as they are with whatever ran before.  A CJ_LANES body runs for lanes 0..63 one after another: the contract's rule (no body reads
// what another lane wrote in the same body) is what makes that the wavefront's result.
#pragma once
#include <setjmp.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/cramjam_hip.h"
#define __device__
#define __host__
#define __forceinline__ inline
#define CJ_LANES(lane) for (uint32_t lane = 0; lane < 64u; lane++)
#define SIM_BOUNDS (-9999)

namespace cj {

struct SimRange {
    const uint8_t *lo = nullptr, *hi = nullptr;
    void set(const void* p, size_t n) { lo = (const uint8_t*)p; hi = lo + n; }
    bool has(const void* p, size_t n) const { return (const uint8_t*)p >= lo && (const uint8_t*)p <= hi && n <= (size_t)(hi - (const uint8_t*)p); }
};
static SimRange sim_in, sim_out, sim_src2, sim_lds, sim_rec;
static jmp_buf sim_jmp;
static bool sim_armed = false;
static bool sim_device_loads = false;        // what InWindow reads outside the stream: false 0xEE, true what load_row loads
static bool sim_ring = false;                // SIM_MAIN: the cases file holds each stream with the neighbour bytes of its edge dwords
extern "C" __attribute__((used, weak, visibility("default"))) void sim_set_device_loads(int on) { sim_device_loads = on != 0; }

[[noreturn]] static void sim_fail() {
    if (!sim_armed) { fprintf(stderr, "sim_fail() outside sim_run()\n"); abort(); }      // (an entry point's mistake, not a decoder's)
    longjmp(sim_jmp, 1);
}
// f() with the stand-ins armed: its value, or SIM_BOUNDS when a check fired (no frame between f and a check may hold a destructor)
template <class F>
static long long sim_run(F&& f) {
    sim_armed = true;
    if (setjmp(sim_jmp)) { sim_armed = false; return SIM_BOUNDS; }
    const long long r = f();
    sim_armed = false;
    return r;
}
static void sim_need(const SimRange& r, const void* p, size_t n) { if (!r.has(p, n)) sim_fail(); }

template <class T>
static T* sim_new_block(size_t bytes = sizeof(T)) {
    T* p = (T*)malloc(bytes ? bytes : 1);
    memset(p, 0xA5, bytes);
    return p;
}

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
        if (sim_device_loads) {                                         // base is a dword boundary: the dword of byte p starts at p & ~3
            for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(((pos + k) & ~3u) < iend ? base[pos + k] : 0) << (8 * k);
            return v;
        }
        for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(base + pos + k >= sim_in.lo && pos + k < iend ? base[pos + k] : 0xEE) << (8 * k);
        return v;
    }
    uint32_t fetch32_any(uint32_t pos) { if (pos - wpos > 500u) anchor(pos); return fetch32(pos); }
};

// a source is the stream or the second range, never a run across both
static void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    if (n == 0) return;
    if ((!sim_in.has(src, n) && !sim_src2.has(src, n)) || !sim_out.has(dst, n)) sim_fail();
    memcpy(dst, src, n);
}
// (one copy of this used to let m == 0 pass with any d; no decoder relies on it: every suite passes under the strict rule)
static void wave_match_copy(uint8_t* dst, uint32_t d, uint32_t m) {
    if (d == 0 || !sim_out.has(dst, m) || (size_t)(dst - sim_out.lo) < d) sim_fail();
    for (uint32_t j = 0; j < m; j++) dst[j] = dst[(int64_t)j - d];
}
static void wave_order() {}

static uint32_t lds_ld(const uint32_t* p) { sim_need(sim_lds, p, 4); return *p; }
static uint32_t lds_ld8(const uint8_t* p) { sim_need(sim_lds, p, 1); return *p; }
static void lds_add(uint32_t* p, uint32_t v) { sim_need(sim_lds, p, 4); *p += v; }
static void lds_xor(uint32_t* p, uint32_t v) { sim_need(sim_lds, p, 4); *p ^= v; }
static void lds_or(uint32_t* p, uint32_t v) { sim_need(sim_lds, p, 4); *p |= v; }
static uint32_t in_ld8(const uint8_t* p) { sim_need(sim_in, p, 1); return *p; }
static uint32_t in_ld32(const uint8_t* p) { sim_need(sim_in, p, 4); uint32_t v; memcpy(&v, p, 4); return v; }
static uint32_t out_ld8(const uint8_t* p) { sim_need(sim_out, p, 1); return *p; }
static uint32_t out_rd32(const uint8_t* p) { sim_need(sim_out, p, 4); uint32_t v; memcpy(&v, p, 4); return v; }
static void out_st8(uint8_t* p, uint32_t v) { sim_need(sim_out, p, 1); *p = (uint8_t)v; }
static void out_st32(uint8_t* p, uint32_t v) { sim_need(sim_out, p, 4); memcpy(p, &v, 4); }
static void slot_st8(uint8_t* p, uint32_t v) { sim_need(sim_src2, p, 1); *p = (uint8_t)v; }
template <class Rec>
static Rec rec_ld(const Rec* slot, uint32_t i) { sim_need(sim_rec, slot + i, sizeof(Rec)); return slot[i]; }      // (the encoder's: Rec = DfeRec)

struct LaneBytes {
    uint8_t v[64];
    void put(uint32_t k, uint32_t byte) { if (k >= 64u) sim_fail(); v[k] = (uint8_t)byte; }
    void flush(uint8_t* dst, uint32_t n) {
        if (n > 64u) sim_fail();
        sim_need(sim_out, dst, n);
        memcpy(dst, v, n);
    }
};
struct LaneU32 { uint32_t v[64]; uint32_t& operator[](uint32_t l) { if (l >= 64u) sim_fail(); return v[l]; } };
struct LaneU64 { uint64_t v[64]; uint64_t& operator[](uint32_t l) { if (l >= 64u) sim_fail(); return v[l]; } };
static uint32_t lane_excl_add(LaneU32& x, LaneU32& before) {
    uint32_t run = 0;
    for (uint32_t l = 0; l < 64u; l++) { before.v[l] = run; run += x.v[l]; }
    return run;
}

// ---- SIM_MAIN: a stand-alone program over a file of cases, the form a sanitizer build takes ------------------------------------------
// A heap block of exactly mis + n bytes, so that a sanitizer sees each edge; p = its byte mis.  With a file, bytes [mis, mis + n) are
// read from it (ok: they were there).  ring: the block is the dwords the stream touches and nothing more — mis & 3 bytes in front and
// the bytes up to the next dword boundary behind, all read from the file: what load_row may load, and a sanitizer sees one byte more.
struct SimBlock {
    uint8_t *mem, *p;
    bool ok;
    SimBlock(FILE* f, size_t n, size_t mis = 0, bool ring = false) {
        const size_t front = ring ? (mis & 3u) : mis, all = ring ? (front + n + 3u) & ~(size_t)3u : front + n;
        mem = (uint8_t*)malloc(all ? all : 1);
        p = mem + front;
        ok = ring ? (all == 0 || fread(mem, 1, all, f) == all) : (!f || n == 0 || fread(p, 1, n, f) == n);
    }
    SimBlock(const SimBlock&) = delete;
    ~SimBlock() { free(mem); }
};
// cases file: u32 count, then per case `nhdr` u32 words | i64 expected result | the blocks that one(f, h, want, got) reads itself.
// one() returns 0 (as expected), 1 (not: got is printed) or 2 (the file is short).
template <class F>
static int sim_cases_main(int argc, char** argv, uint32_t nhdr, F&& one) {
    FILE* f = argc < 2 ? nullptr : fopen(argv[1], "rb");
    sim_ring = sim_device_loads = argc > 2 && strcmp(argv[2], "device") == 0;
    uint32_t count = 0, bad = 0, h[8];
    if (!f || nhdr > 8u || fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        int64_t want;
        long long got = 0;
        if (fread(h, 4, nhdr, f) != nhdr || fread(&want, 8, 1, f) != 1) return 2;
        const int st = one(f, h, want, got);
        if (st == 2) return 2;
        if (st) { bad++; printf("case %u: got %lld want %lld\n", c, got, (long long)want); }
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}

}  // namespace cj
