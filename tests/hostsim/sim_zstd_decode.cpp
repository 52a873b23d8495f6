// zstd_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_zstd_model.py (and, with SIM_MAIN, a
// stand-alone program that runs a file of cases).  The literal slot is the second source range.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/zstd_wave.hpp"

// size != 0: the size query (out, cap and the slot are not used)
extern "C" long long sim_zstd_decode(int size, const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::ZstdLds* L = cj::sim_new_block<cj::ZstdLds>();
    uint8_t* slot = cj::sim_new_block<uint8_t>(cj::kZsSlotBytes);
    cj::sim_in.set(in, n); cj::sim_out.set(out, size ? 0 : cap); cj::sim_src2.set(slot, size ? 0 : cj::kZsSlotBytes); cj::sim_lds.set(L, sizeof *L);
    const long long r = cj::sim_run([&]() -> long long {
        return size ? cj::zstd_wave_decode<true>(in, n, nullptr, 0, L, nullptr) : cj::zstd_wave_decode<false>(in, n, out, cap, L, slot);
    });
    free(L);
    free(slot);
    return r;
}

// *h = XXH64(p[0, n), seed 0) as the lanes compute it (tests compare it with a scalar one); 0 or SIM_BOUNDS
extern "C" long long sim_zstd_xxh64(unsigned char* p, unsigned int n, unsigned long long* h) {
    cj::ZstdLds* L = cj::sim_new_block<cj::ZstdLds>();
    cj::sim_out.set(p, n); cj::sim_lds.set(L, sizeof *L);
    const long long r = cj::sim_run([&] { *h = cj::zs_xxh64(L, p, n); return 0; });
    free(L);
    return r;
}

extern "C" unsigned int sim_zstd_lds_bytes(void) { return (unsigned int)sizeof(cj::ZstdLds); }

#ifdef SIM_MAIN
// per case u32 size, n, cap, mis | i64 expected result | stream | expected bytes (decode mode, result > 0)
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 4, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = (!h[0] && want > 0) ? (size_t)want : 0;
        cj::SimBlock in(f, h[1], h[3], cj::sim_ring), exp(f, nexp), out(nullptr, h[2]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_zstd_decode((int)h[0], in.p, h[1], out.p, h[2]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
