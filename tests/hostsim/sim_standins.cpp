// The stand-ins of sim_wave.hpp themselves, for tests/test_hostsim_standins.py: one access per call inside an arena of 256 bytes
// (byte i = i before every call) whose ranges lie with gaps around them, so that an access a check wrongly let through still lands in
// the arena:  rec [16, 48): two records of 16 bytes   in [64, 104)   src2 [104, 128) right behind it   out [160, 208)   lds [224, 256).
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/wave_window.hpp"

using namespace cj;

static uint32_t g_arena32[64];
static uint8_t* const A = (uint8_t*)g_arena32;
struct Rec { uint32_t a, b, c, d; };
enum { REC = 16, REC_N = 32, IN = 64, IN_N = 40, SRC2 = 104, SRC2_N = 24, OUT = 160, OUT_N = 48, LDS = 224, LDS_N = 32 };

extern "C" void standin_arena(unsigned char* dst) { memcpy(dst, A, 256); }

// a, b, c: offsets are relative to the op's own range (wave_copy's source: to the arena)
extern "C" long long standin(int op, long a, long b, long c) {
    for (int i = 0; i < 256; i++) A[i] = (uint8_t)i;
    sim_device_loads = false;
    sim_in.set(A + IN, IN_N); sim_src2.set(A + SRC2, SRC2_N); sim_out.set(A + OUT, OUT_N); sim_lds.set(A + LDS, LDS_N); sim_rec.set(A + REC, REC_N);
    return sim_run([&]() -> long long {
        switch (op) {
        case 0: return in_ld8(A + IN + a);
        case 1: return in_ld32(A + IN + a);
        case 2: return out_ld8(A + OUT + a);
        case 3: return out_rd32(A + OUT + a);
        case 4: out_st8(A + OUT + a, (uint32_t)b); return 0;
        case 5: out_st32(A + OUT + a, (uint32_t)b); return 0;
        case 6: slot_st8(A + SRC2 + a, (uint32_t)b); return 0;
        case 7: return lds_ld((const uint32_t*)(A + LDS + a));
        case 8: return lds_ld8(A + LDS + a);
        case 9: lds_add((uint32_t*)(A + LDS + a), (uint32_t)b); return 0;
        case 10: lds_xor((uint32_t*)(A + LDS + a), (uint32_t)b); return 0;
        case 11: lds_or((uint32_t*)(A + LDS + a), (uint32_t)b); return 0;
        case 12: wave_copy(A + OUT + a, A + b, (uint32_t)c); return 0;
        case 13: wave_match_copy(A + OUT + a, (uint32_t)b, (uint32_t)c); return 0;
        case 14: { LaneBytes lb; lb.put((uint32_t)a, (uint32_t)b); return lb.v[a & 63]; }
        case 15: { LaneBytes lb; for (uint32_t k = 0; k < 64u; k++) lb.put(k, k ^ 0x5Au); lb.flush(A + OUT + a, (uint32_t)b); return 0; }
        case 16: { InWindow w; w.base = A; w.iend = IN + IN_N; w.anchor((uint32_t)a); return w.fetch32((uint32_t)b); }      // (positions: arena offsets)
        case 17: { InWindow w; const uint32_t mis = window_open(w, A + IN + a, (uint32_t)b); return (long long)mis | (long long)(w.base - A) << 8 | (long long)w.iend << 16 | (long long)w.wpos << 32; }
        case 18: { LaneU32 x = {}; x[(uint32_t)a] = 7u; return x.v[a & 63]; }
        case 19: { LaneU64 x = {}; x[(uint32_t)a] = 7u; return (long long)x.v[a & 63]; }
        case 20: { LaneU32 x, before; for (uint32_t l = 0; l < 64u; l++) x[l] = l + 1u; const uint32_t t = lane_excl_add(x, before); return (long long)t << 32 | before[(uint32_t)a]; }
        case 21: return rec_ld((const Rec*)(A + REC + a), (uint32_t)b).d;      // a: bytes from the range's start, b: the record's index
        // the device-load mode: a stream of b bytes that begins a (0..3) bytes behind the dword boundary A + IN; c: the position relative to it
        case 22: { InWindow w; w.base = A + IN; w.iend = (uint32_t)(a + b); w.anchor(0); sim_device_loads = true; return w.fetch32((uint32_t)c); }
        }
        return -1;
    });
}
