// snappy_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_input_sweep_model.py and
// tests/test_neighbours_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases).  Literals come from the stream,
// copies from the output: nothing else is a source.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/snappy_wave.hpp"

extern "C" long long sim_snappy_wave_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::sim_in.set(in, n); cj::sim_out.set(out, cap); cj::sim_src2.set(nullptr, 0);
    return cj::sim_run([&] { return cj::snappy_wave_decode(in, n, out, cap); });
}

#ifdef SIM_MAIN
// per case u32 n, cap, mis_in | i64 expected result | stream | expected bytes
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 3, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        cj::SimBlock in(f, h[0], h[2], cj::sim_ring), exp(f, nexp), out(nullptr, h[1]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_snappy_wave_decode(in.p, h[0], out.p, h[1]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
