// deflate_enc_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_deflate_encode_model.py (and, with
// SIM_MAIN, a stand-alone program that runs a file of cases).  The matcher is the model's (deflate_enc_model.c: dfe_model_records,
// linked in) — on the device it is enc2::Walk<RecFmt<32768>, 2>, held to the same records by the GPU tests.  The input range is the
// piece, the record range what the matcher wrote of a slot that is a heap block of exactly what the piece may need.
#include "sim_wave.hpp"

extern "C" uint32_t dfe_model_records(const uint8_t* in, uint32_t n, uint32_t* rec);

#include "../../cramjam_amd/csrc/deflate_enc_wave.hpp"
#include "../../cramjam_amd/csrc/crc32_lanes.hpp"

static cj::DfeLds* new_lds() {
    cj::DfeLds* L = cj::sim_new_block<cj::DfeLds>();
    cj::sim_lds.set(L, sizeof *L);
    return L;
}

static uint32_t adler32_of(const uint8_t* p, uint64_t n) {
    uint32_t a = 1, b = 0;
    for (uint64_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
static uint32_t crc32_of(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? cj::kCrc32Poly : 0u); }
    return ~c;
}

// One stream, as the kernel's first wavefront walks it.  types (may be null): the block type of every piece
extern "C" long long sim_deflate_encode(int wrap, const unsigned char* in, unsigned long long n, unsigned char* out, unsigned long long cap64, unsigned char* types) {
    if (n > cj::kDfeInMax) return CJ_E_INPUT_TOO_LARGE;
    cj::DfeLds* L = new_lds();
    const uint32_t cap = (uint32_t)(cap64 < 0xFFFFFFF0ull ? cap64 : 0xFFFFFFF0ull);
    cj::sim_out.set(out, cap);
    cj::DfeRec* volatile slot = nullptr;              // (freed behind a check that fired, too)
    const long long r = cj::sim_run([&]() -> long long {
        cj::DfeOut W;
        bool ok = cj::dfe_begin(L, W, wrap, out, cap);
        const uint64_t np = n == 0 ? 1 : (n + cj::kDfePiece - 1) / cj::kDfePiece;
        for (uint64_t p = 0; p < np && ok; p++) {
            const uint8_t* pin = in + p * cj::kDfePiece;
            const uint32_t pn = (uint32_t)(n - p * cj::kDfePiece < cj::kDfePiece ? n - p * cj::kDfePiece : cj::kDfePiece);
            slot = (cj::DfeRec*)malloc(sizeof(cj::DfeRec) * (pn / 4u + 2u));      // exactly what this piece may need
            const uint32_t nrec = dfe_model_records(pin, pn, (uint32_t*)slot);
            cj::sim_in.set(pin, pn);
            cj::sim_rec.set(slot, sizeof(cj::DfeRec) * nrec);
            uint32_t t = 0;
            ok = cj::dfe_piece(L, W, pin, pn, slot, nrec, p + 1 == np, cj::dfe_tail_bytes(wrap), &t);
            if (types) types[p] = (unsigned char)t;
            free(slot);
            slot = nullptr;
        }
        if (!ok) return CJ_E_OUT_TOO_SMALL;
        return cj::dfe_end(L, W, wrap, wrap == cj::kDfeZlib ? adler32_of(in, n) : wrap == cj::kDfeGzip ? crc32_of(in, n) : 0u, (uint32_t)n);
    });
    free(slot);
    free(L);
    return r;
}

// the code builder alone: lens[0, nsym) from hist[0, nsym); 0 or SIM_BOUNDS
extern "C" long long sim_dfe_build_lens(const unsigned int* hist, unsigned int nsym, unsigned int maxbits, int pad_single, unsigned char* lens) {
    cj::DfeLds* L = new_lds();
    for (uint32_t s = 0; s < nsym && s < 288u; s++) L->hist[s] = hist[s];
    const long long r = cj::sim_run([&] { cj::dfe_build_lens(L, L->hist, nsym, maxbits, pad_single != 0, L->lens); return 0; });
    memcpy(lens, L->lens, nsym);
    free(L);
    return r;
}
// ... and the canonical codes of given lengths: code[s] = bit-reversed code | length << 16; 0 or SIM_BOUNDS
extern "C" long long sim_dfe_assign_codes(const unsigned char* lens, unsigned int nsym, unsigned int maxbits, unsigned int* code) {
    cj::DfeLds* L = new_lds();
    memcpy(L->lens, lens, nsym);
    const long long r = cj::sim_run([&] { cj::dfe_assign_codes(L, L->lens, nsym, maxbits, L->code); return 0; });
    memcpy(code, L->code, 4u * nsym);
    free(L);
    return r;
}
extern "C" unsigned long long sim_dfe_bound(unsigned long long n, int wrap) { return cj::dfe_bound(n, wrap); }

#ifdef SIM_MAIN
// per case u32 wrap, n, cap, in_mis, out_mis | i64 expected result | input | expected stream (result > 0)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 5, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        cj::SimBlock in(f, h[1], h[3]), exp(f, nexp), out(nullptr, h[2], h[4]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_deflate_encode((int)h[0], in.p, h[1], out.p, h[2], nullptr);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
