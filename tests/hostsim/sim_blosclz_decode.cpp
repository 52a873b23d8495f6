// blosclz_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_blosclz_model.py.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/blosclz_wave.hpp"

extern "C" long long sim_blosclz_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::sim_in.set(in, n); cj::sim_out.set(out, cap);
    return cj::sim_run([&] { return cj::blosclz_wave_decode(in, n, out, cap); });
}

#ifdef SIM_MAIN
// per case u32 n, cap, mis | i64 expected result | stream | expected bytes (result > 0)
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 3, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        cj::SimBlock in(f, h[0], h[2], cj::sim_ring), exp(f, nexp), out(nullptr, h[1]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_blosclz_decode(in.p, h[0], out.p, h[1]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
