// deflate_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_deflate_model.py (and, with SIM_MAIN, a
// stand-alone program that runs a file of cases).
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/deflate_wave.hpp"

static const cj::Crc32Tables g_crc = cj::make_crc32_tables();

// wrap: a cj_deflate_wrap; size != 0: the size query (out and cap are not used)
extern "C" long long sim_deflate_decode(int wrap, int size, const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::DeflateLds* L = cj::sim_new_block<cj::DeflateLds>();
    cj::sim_in.set(in, n); cj::sim_out.set(out, size ? 0 : cap); cj::sim_lds.set(L, sizeof *L);
    const uint32_t* adv = &g_crc.adv256[0][0];
    const long long r = cj::sim_run([&]() -> long long {
        if (!size) {
            if (wrap == 0) return cj::deflate_wave_decode<0, false>(in, n, out, cap, L, adv, g_crc.xpow8);
            if (wrap == 1) return cj::deflate_wave_decode<1, false>(in, n, out, cap, L, adv, g_crc.xpow8);
            if (wrap == 2) return cj::deflate_wave_decode<2, false>(in, n, out, cap, L, adv, g_crc.xpow8);
        } else {
            if (wrap == 0) return cj::deflate_wave_decode<0, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
            if (wrap == 1) return cj::deflate_wave_decode<1, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
            if (wrap == 2) return cj::deflate_wave_decode<2, true>(in, n, nullptr, 0, L, adv, g_crc.xpow8);
        }
        return CJ_E_BAD_ARG;
    });
    free(L);
    return r;
}

#ifdef SIM_MAIN
// per case u32 wrap, size, n, cap, mis | i64 expected result | stream | expected bytes (decode mode, result > 0)
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 5, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = (!h[1] && want > 0) ? (size_t)want : 0;
        cj::SimBlock in(f, h[2], h[4], cj::sim_ring), exp(f, nexp), out(nullptr, h[3]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_deflate_decode((int)h[0], (int)h[1], in.p, h[2], out.p, h[3]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
