// Host build of the LZ4 size walk (cramjam_amd/csrc/lz4_size_walk.hpp) for tests/test_batch_sizes_model.py: the scalar statement of
// what cj_batch_sizes_device's kernels decide per sequence, compiled as a stand-alone program under AddressSanitizer + UBSan.
// Every block is copied into a heap buffer of exactly its size, so a read past either end of the input is reported.
// stdin:  records of  u32 length (little endian) + that many bytes.   stdout: one line per record, the walk's result.
// This is a TEST of product source, not a CPU codec: nothing in cramjam_amd links it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../cramjam_amd/csrc/lz4_size_walk.hpp"

static int64_t size_of(const uint8_t* in, uint64_t n) {
    if (n == 0 || n > cj::kLz4InMax) return CJ_E_CORRUPT;
    const uint32_t iend = (uint32_t)n;
    const auto rd = [&](uint32_t p) -> uint32_t {          // 4 bytes at p, zero-filled past the end
        uint32_t v = 0;
        if (p + 4u <= iend) { memcpy(&v, in + p, 4); return v; }
        for (uint32_t i = 0; i < 4u && p + i < iend; i++) v |= (uint32_t)in[p + i] << (8u * i);
        return v;
    };
    const auto ff = [&](uint32_t p, uint32_t e) { return cj::lz4_ff_run(in, p, e); };
    return cj::lz4_size_walk(rd, ff, 0u, iend);
}

int main() {
    for (;;) {
        uint8_t hdr[4];
        if (fread(hdr, 1, 4, stdin) != 4) break;
        const uint32_t n = (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) | ((uint32_t)hdr[3] << 24);
        uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
        if (n && fread(buf, 1, n, stdin) != n) { fprintf(stderr, "short record\n"); return 2; }
        uint8_t* exact = (uint8_t*)malloc(n);               // (n == 0: a zero-size block — any read is out of bounds)
        if (n) memcpy(exact, buf, n);
        printf("%lld\n", (long long)size_of(exact, n));
        free(exact); free(buf);
    }
    return 0;
}
