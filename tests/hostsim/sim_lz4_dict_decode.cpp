// lz4_dict_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_lz4_dict_model.py (and, with SIM_MAIN,
// a stand-alone program that runs a file of cases).  Literals come from the stream, the head of a match from the dictionary's counted
// tail (the second source range): nothing else is a source.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/lz4_dict_wave.hpp"

// dict / dict_len: the whole dictionary; the decoder gets its end and min(dict_len, 65536), as the kernel does
extern "C" long long sim_lz4_dict_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap, const unsigned char* dict,
                                         unsigned int dict_len) {
    const unsigned int hist = dict_len < 65536u ? dict_len : 65536u;
    cj::sim_in.set(in, n); cj::sim_out.set(out, cap); cj::sim_src2.set(dict + dict_len - hist, hist);
    return cj::sim_run([&] { return cj::lz4_dict_wave_decode(in, n, out, cap, dict + dict_len, hist); });
}

#ifdef SIM_MAIN
// per case u32 n, cap, dict_len, mis_in, mis_dict | i64 expected result | stream | dictionary | expected bytes
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 5, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        cj::SimBlock in(f, h[0], h[3], cj::sim_ring), d(f, h[2], h[4]), exp(f, nexp), out(nullptr, h[1]);
        if (!in.ok || !d.ok || !exp.ok) return 2;
        got = sim_lz4_dict_decode(in.p, h[0], out.p, h[1], d.p, h[2]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
