// lz4_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_lz4_dict_model.py, tests/test_input_sweep_model.py
// and tests/test_neighbours_model.py (and, with SIM_MAIN, a stand-alone program that runs a file of cases).  Literals come from the
// stream; the head of a dictionary match from the dictionary's counted tail (the second source range); a plain or linked match from the
// output and the history directly in front of it: nothing else is a source.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/lz4_wave.hpp"

// <true>, lz4_dict_decode_kernel's.  dict / dict_len: the whole dictionary; the decoder gets its end and min(dict_len, 65536), as the kernel does
extern "C" long long sim_lz4_dict_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap, const unsigned char* dict,
                                         unsigned int dict_len) {
    const unsigned int hist = dict_len < 65536u ? dict_len : 65536u;
    cj::sim_in.set(in, n); cj::sim_out.set(out, cap); cj::sim_src2.set(dict + dict_len - hist, hist);
    return cj::sim_run([&] { return cj::lz4_wave_decode<true>(in, n, out, cap, dict + dict_len, hist); });
}

// <false>, lz4_decode_kernel's (hist = 0) and lz4_frame_chain_kernel's: the hist bytes in front of `out` are output written before
extern "C" long long sim_lz4_wave_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap, unsigned int hist) {
    cj::sim_in.set(in, n); cj::sim_out.set(out - hist, (size_t)hist + cap); cj::sim_src2.set(nullptr, 0);
    return cj::sim_run([&] { return cj::lz4_wave_decode<false>(in, n, out, cap, nullptr, hist); });
}

#ifdef SIM_MAIN
// per case u32 n, cap, dict_len, mis_in, mis_dict, linked | i64 expected result | stream | dictionary | expected bytes
// linked = 0: the dictionary entry; 1: the plain entry with the dict_len bytes as history in front of the output block (mis_dict unused)
// (a second argument `device`: the device-load mode, and the stream comes with the neighbour bytes of its first and last dword)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 6, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        if (h[5]) {
            cj::SimBlock in(f, h[0], h[3], cj::sim_ring), hist(f, h[2]), exp(f, nexp), out(nullptr, (size_t)h[2] + h[1]);      // out: history | cap bytes
            if (!in.ok || !hist.ok || !exp.ok) return 2;
            memcpy(out.p, hist.p, h[2]);
            got = sim_lz4_wave_decode(in.p, h[0], out.p + h[2], h[1], h[2]);
            return (int)(got != want || (nexp && memcmp(out.p + h[2], exp.p, nexp) != 0) || (h[2] && memcmp(out.p, hist.p, h[2]) != 0));
        }
        cj::SimBlock in(f, h[0], h[3], cj::sim_ring), d(f, h[2], h[4]), exp(f, nexp), out(nullptr, h[1]);
        if (!in.ok || !d.ok || !exp.ok) return 2;
        got = sim_lz4_dict_decode(in.p, h[0], out.p, h[1], d.p, h[2]);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
