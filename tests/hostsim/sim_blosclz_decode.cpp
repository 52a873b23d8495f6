// blosclz_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_blosclz_model.py.
#include "sim_wave.hpp"
#include "../../cramjam_amd/csrc/blosclz_wave.hpp"

extern "C" long long sim_blosclz_decode(const unsigned char* in, unsigned int n, unsigned char* out, unsigned int cap) {
    cj::sim_in.set(in, n); cj::sim_out.set(out, cap);
    return cj::sim_run([&] { return cj::blosclz_wave_decode(in, n, out, cap); });
}
