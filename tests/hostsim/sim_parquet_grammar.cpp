// parquet_grammar.hpp compiled for the host, unchanged: the page table and the verdict of the page walk, for tests/test_parquet_model.py —
// as a shared object for ctypes, or (SIM_MAIN) as a stand-alone program over a file of cases, the form the sanitizer build takes.
#include "../../cramjam_amd/csrc/parquet_grammar.hpp"

extern "C" {

// rows: the 8 words of the pages query per page; returns the walk's code, *n_pages = pages visited
long long sim_pq_walk(const unsigned char* in, unsigned long long n, long long* rows, unsigned long long max_rows, unsigned long long* n_pages) {
    unsigned long long k = 0, run = 0;
    const long long err = cj::pq_walk(in, (size_t)n, [&](const cj::PqPage& pg) {
        if (k < max_rows) {
            int64_t w[cj::kPqPageWords];
            pg.words(run, w);
            for (size_t j = 0; j < cj::kPqPageWords; j++) rows[cj::kPqPageWords * k + j] = w[j];
        }
        k++; run += pg.decoded();
    });
    *n_pages = k;
    return err;
}

int sim_pq_skip_depth() { return cj::kPqSkipDepth; }

}

#ifdef SIM_MAIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
// The file: u32 count, then per case u32 n, u32 pages | i64 expected code | the chunk | per page 8 x i64.  Every chunk is a heap block
// of exactly n bytes — it lies flush against the end of its allocation, so a read behind n is the sanitizer's.
int main(int argc, char** argv) {
    FILE* f = argc < 2 ? nullptr : fopen(argv[1], "rb");
    uint32_t count = 0, bad = 0, h[2];
    if (!f || fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        int64_t want;
        if (fread(h, 4, 2, f) != 2 || fread(&want, 8, 1, f) != 1) return 2;
        const uint32_t n = h[0], np = h[1];
        uint8_t* in = (uint8_t*)malloc(n);                     // (n = 0: the walk reads nothing; whatever malloc gives is not touched)
        long long* exp = (long long*)malloc(64 * (size_t)np + 8);
        long long* got = (long long*)malloc(64 * (size_t)np + 8);
        if ((n && fread(in, 1, n, f) != n) || (np && fread(exp, 64, np, f) != np)) return 2;
        unsigned long long k = 0;
        const long long r = sim_pq_walk(in, n, got, np, &k);
        const bool ok = r == want && k == np && (np == 0 || memcmp(got, exp, 64 * (size_t)np) == 0) && k <= n;
        if (!ok) { bad++; printf("case %u: got %lld with %llu pages, want %lld with %u\n", c, r, k, (long long)want, np); }
        free(in); free(exp); free(got);
    }
    fclose(f);
    printf("%u cases, %u bad\n", count, bad);
    return bad ? 1 : 0;
}
#endif
