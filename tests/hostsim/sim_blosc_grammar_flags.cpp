// blosc_grammar.hpp compiled for the host with a caller's flags word (CJ_BLOSC_FLAG_READ_*): the stream list, the header and the
// verdict of the chunk walk, for tests/test_blosc_zcodecs_model.py.  sim_blosc_grammar.cpp is the same walk under the default reading.
#include "../../cramjam_amd/csrc/blosc_grammar.hpp"

extern "C" {

// rows: 6 uint32 per stream (src_off, src_len, dst_off, dst_len, block, stored); hdr9: the header's eight words and the format the walk
// reports; returns the walk's code, *n_streams = streams seen
long long sim_blosc_walk_flags(const unsigned char* in, unsigned long long n, unsigned int read_flags, unsigned int* hdr9, unsigned int* rows,
                               unsigned long long max_rows, unsigned long long* n_streams) {
    cj::BloscHeader h;
    unsigned long long k = 0;
    const long long err = cj::blosc_walk(in, (size_t)n, h, [&](const cj::BloscStream& s) {
        if (k < max_rows) {
            unsigned int* r = rows + 6 * k;
            r[0] = s.src_off; r[1] = s.src_len; r[2] = s.dst_off; r[3] = s.dst_len; r[4] = s.block; r[5] = s.stored ? 1u : 0u;
        }
        k++;
    }, read_flags);
    const unsigned int v[9] = { h.version, h.versionlz, h.flags, h.typesize, h.nbytes, h.blocksize, h.cbytes, h.nblocks, h.format };
    for (int i = 0; i < 9; i++) hdr9[i] = v[i];
    *n_streams = k;
    return err;
}

// blosc_header alone with the flags word
long long sim_blosc_header_flags(const unsigned char* in, unsigned long long n, unsigned int read_flags) {
    cj::BloscHeader h;
    return cj::blosc_header(in, (size_t)n, h, read_flags);
}

}
