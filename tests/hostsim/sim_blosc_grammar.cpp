// blosc_grammar.hpp compiled for the host: the stream list and the verdict of the chunk walk, for tests/test_blosc_model.py
// (built there with -fsanitize=address,undefined: a read outside the chunk is a test failure)
#include "../../cramjam_amd/csrc/blosc_grammar.hpp"

extern "C" {

// rows: 6 uint32 per stream (src_off, src_len, dst_off, dst_len, block, stored); returns the walk's code, *n_streams = streams seen
long long sim_blosc_walk(const unsigned char* in, unsigned long long n, unsigned int* hdr8, unsigned int* rows, unsigned long long max_rows,
                         unsigned long long* n_streams) {
    cj::BloscHeader h;
    unsigned long long k = 0;
    const long long err = cj::blosc_walk(in, (size_t)n, h, [&](const cj::BloscStream& s) {
        if (k < max_rows) {
            unsigned int* r = rows + 6 * k;
            r[0] = s.src_off; r[1] = s.src_len; r[2] = s.dst_off; r[3] = s.dst_len; r[4] = s.block; r[5] = s.stored ? 1u : 0u;
        }
        k++;
    });
    const unsigned int v[8] = { h.version, h.versionlz, h.flags, h.typesize, h.nbytes, h.blocksize, h.cbytes, h.nblocks };
    for (int i = 0; i < 8; i++) hdr8[i] = v[i];
    *n_streams = k;
    return err;
}

unsigned int sim_blosc_block_mode(unsigned int flags, unsigned int typesize, unsigned int bytes) { return cj::blosc_block_mode(flags, typesize, bytes); }
unsigned long long sim_blosc_tr8(unsigned long long x) { return cj::blosc_tr8(x); }
void sim_blosc_layout(unsigned int nbytes, unsigned int typesize, unsigned int want, unsigned int* out3) {
    const cj::BloscLayout l = cj::blosc_layout(nbytes, typesize, want);
    out3[0] = l.blocksize; out3[1] = l.nblocks; out3[2] = l.split ? 1u : 0u;
}

}
