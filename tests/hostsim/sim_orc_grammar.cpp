// orc_grammar.hpp compiled for the host, unchanged: the chunk list and the verdict of the hop walk, for tests/test_orc_model.py —
// as a shared object for ctypes, or (SIM_MAIN) as a stand-alone program over a file of cases, the form the sanitizer build takes.
#include "../../cramjam_amd/csrc/orc_grammar.hpp"

extern "C" {

// rows: 3 uint64 per chunk (offset of its bytes, their length, original); returns the walk's code, *n_chunks = chunks visited
long long sim_orc_walk(const unsigned char* in, unsigned long long n, unsigned long long* rows, unsigned long long max_rows,
                       unsigned long long* n_chunks) {
    unsigned long long k = 0;
    const long long err = cj::orc_walk(in, (size_t)n, [&](uint64_t off, uint32_t len, bool orig) {
        if (k < max_rows) { rows[3 * k] = off; rows[3 * k + 1] = len; rows[3 * k + 2] = orig ? 1u : 0u; }
        k++;
    });
    *n_chunks = k;
    return err;
}

unsigned long long sim_orc_bound(unsigned long long n, unsigned long long block_size) { return cj::orc_bound(n, block_size); }

}

#ifdef SIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
// The file: u32 count, then per case u32 n, u32 chunks | i64 expected code | the stream | per chunk u64 offset, length, original.  Every
// stream is a heap block of exactly n bytes — it lies flush against the end of its allocation, so a read behind n is the sanitizer's.
int main(int argc, char** argv) {
    FILE* f = argc < 2 ? nullptr : fopen(argv[1], "rb");
    uint32_t count = 0, bad = 0, h[2];
    if (!f || fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        int64_t want;
        if (fread(h, 4, 2, f) != 2 || fread(&want, 8, 1, f) != 1) return 2;
        const uint32_t n = h[0], nc = h[1];
        uint8_t* in = (uint8_t*)malloc(n);                     // (n = 0: the walk reads nothing; whatever malloc gives is not touched)
        uint64_t* exp = (uint64_t*)malloc(24 * (size_t)nc + 8);
        uint64_t* got = (uint64_t*)malloc(24 * (size_t)nc + 8);
        if ((n && fread(in, 1, n, f) != n) || (nc && fread(exp, 24, nc, f) != nc)) return 2;
        unsigned long long k = 0;
        const long long r = sim_orc_walk(in, n, (unsigned long long*)got, nc, &k);
        const bool ok = r == want && k == nc && (nc == 0 || memcmp(got, exp, 24 * (size_t)nc) == 0) && k <= n / 3;
        if (!ok) { bad++; printf("case %u: got %lld with %llu chunks, want %lld with %u\n", c, r, k, (long long)want, nc); }
        free(in); free(exp); free(got);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
