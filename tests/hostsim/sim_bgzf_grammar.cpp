// bgzf_grammar.hpp compiled for the host, unchanged: the member list and the verdict of the hop walk, for tests/test_bgzf_model.py —
// as a shared object for ctypes, or (SIM_MAIN) as a stand-alone program over a file of cases, the form the sanitizer build takes.
#include "../../cramjam_amd/csrc/bgzf_grammar.hpp"

extern "C" {

// rows: 3 uint64 per member (offset, length, ISIZE); returns the walk's code, *n_members = members visited
long long sim_bgzf_walk(const unsigned char* in, unsigned long long n, unsigned long long* rows, unsigned long long max_rows,
                        unsigned long long* n_members) {
    unsigned long long k = 0;
    const long long err = cj::bgzf_walk(in, (size_t)n, [&](uint64_t off, uint32_t len, uint32_t isize) {
        if (k < max_rows) { rows[3 * k] = off; rows[3 * k + 1] = len; rows[3 * k + 2] = isize; }
        k++;
    });
    *n_members = k;
    return err;
}

}

#ifdef SIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
// The file: u32 count, then per case u32 n, u32 members | i64 expected code | the stream | per member u64 offset, length, ISIZE.  Every
// stream is a heap block of exactly n bytes — it lies flush against the end of its allocation, so a read behind n is the sanitizer's.
int main(int argc, char** argv) {
    FILE* f = argc < 2 ? nullptr : fopen(argv[1], "rb");
    uint32_t count = 0, bad = 0, h[2];
    if (!f || fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        int64_t want;
        if (fread(h, 4, 2, f) != 2 || fread(&want, 8, 1, f) != 1) return 2;
        const uint32_t n = h[0], nm = h[1];
        uint8_t* in = (uint8_t*)malloc(n);                     // (n = 0: the walk reads nothing; whatever malloc gives is not touched)
        uint64_t* exp = (uint64_t*)malloc(24 * (size_t)nm + 8);
        uint64_t* got = (uint64_t*)malloc(24 * (size_t)nm + 8);
        if ((n && fread(in, 1, n, f) != n) || (nm && fread(exp, 24, nm, f) != nm)) return 2;
        unsigned long long k = 0;
        const long long r = sim_bgzf_walk(in, n, (unsigned long long*)got, nm, &k);
        const bool ok = r == want && k == nm && (nm == 0 || memcmp(got, exp, 24 * (size_t)nm) == 0) && k <= n / 26 + 1;
        if (!ok) { bad++; printf("case %u: got %lld with %llu members, want %lld with %u\n", c, r, k, (long long)want, nm); }
        free(in); free(exp); free(got);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
