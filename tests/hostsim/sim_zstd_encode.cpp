// zstd_enc_wave.hpp compiled for the host over sim_wave.hpp's checked stand-ins, for tests/test_zstd_encode_model.py (and, with
// SIM_MAIN, a stand-alone program that runs a file of cases).  The matcher is the model's (zstd_enc_model.c: zse_model_records,
// linked in) — on the device it is enc2::Walk<RecFmt<65535>, 2>, held to the same records by the GPU tests.  The input range is the piece,
// the record range what the matcher wrote of a slot that is a heap block of exactly what the piece may need, the literal area
// (sim_src2) a heap block of the piece's length.
#include "sim_wave.hpp"

extern "C" uint32_t zse_model_records(const uint8_t* in, uint32_t n, uint32_t* rec);

namespace cj {
struct DfeRec;
static void rec_st32(DfeRec* slot, uint32_t i, uint32_t w, uint32_t v) {
    uint8_t* p = (uint8_t*)slot + 16u * (size_t)i + 4u * w;
    if (w >= 4u) sim_fail();
    sim_need(sim_rec, p, 4);
    memcpy(p, &v, 4);
}
static uint32_t lit_ld8(const uint8_t* p) { sim_need(sim_src2, p, 1); return *p; }
static void lit_st8(uint8_t* p, uint32_t v) { sim_need(sim_src2, p, 1); *p = (uint8_t)v; }
}  // namespace cj

#include "../../cramjam_amd/csrc/zstd_enc_wave.hpp"

static cj::ZseLds* new_lds() {
    cj::ZseLds* L = cj::sim_new_block<cj::ZseLds>();
    cj::sim_lds.set(L, sizeof *L);
    return L;
}

// One frame, as the kernel's first wavefront walks it (the checksum as its second does).  report (may be null): kZseInfo words a piece
extern "C" long long sim_zstd_encode(unsigned int flags, const unsigned char* in, unsigned long long n, unsigned char* out, unsigned long long cap64,
                                     unsigned int* report) {
    if (n > cj::kZseInMax) return CJ_E_INPUT_TOO_LARGE;
    cj::ZseLds* L = new_lds();
    const uint32_t cap = (uint32_t)(cap64 < 0xFFFFFFF0ull ? cap64 : 0xFFFFFFF0ull);
    cj::sim_out.set(out, cap);
    cj::DfeRec* volatile slot = nullptr;              // (freed behind a check that fired, too)
    uint8_t* volatile lit = nullptr;
    const long long r = cj::sim_run([&]() -> long long {
        cj::ZseOut O;
        bool ok = cj::zse_begin(O, out, cap, (uint32_t)n, flags);
        uint32_t prev = 1u;
        const uint64_t np = n == 0 ? 1 : (n + cj::kZsePiece - 1) / cj::kZsePiece;
        for (uint64_t p = 0; p < np && ok; p++) {
            const uint8_t* pin = in + p * cj::kZsePiece;
            const uint32_t pn = (uint32_t)(n - p * cj::kZsePiece < cj::kZsePiece ? n - p * cj::kZsePiece : cj::kZsePiece);
            slot = (cj::DfeRec*)malloc(sizeof(cj::DfeRec) * (pn / 4u + 2u));      // exactly what this piece may need
            lit = (uint8_t*)malloc(pn ? pn : 1);
            const uint32_t nrec = zse_model_records(pin, pn, (uint32_t*)slot);
            cj::sim_in.set(pin, pn);
            cj::sim_rec.set(slot, sizeof(cj::DfeRec) * nrec);
            cj::sim_src2.set(lit, pn);
            ok = cj::zse_piece(L, O, pin, pn, slot, nrec, lit, p + 1 == np, (flags & cj::kZseChecksum) ? 4u : 0u, prev, report ? report + cj::kZseInfo * p : nullptr);
            free(slot); free(lit);
            slot = nullptr; lit = nullptr;
        }
        if (!ok) return CJ_E_OUT_TOO_SMALL;
        uint64_t x = 0;
        if (flags & cj::kZseChecksum) {
            cj::sim_in.set(in, n);
            x = cj::zse_xxh64(L->acc, in, (uint32_t)n);
        }
        return cj::zse_end(O, flags, x);
    });
    free(slot); free(lit);
    free(L);
    return r;
}

// the table builder alone: table t (0 LL, 1 OF, 2 ML) of the predefined distribution — its 1 << log states, and deltaNbBits /
// deltaFindState of its symbols (64 words each); returns the table's log, or SIM_BOUNDS
extern "C" long long sim_zse_table(unsigned int t, unsigned short* st, unsigned int* dnb, int* dfs) {
    if (t > 2u) return CJ_E_BAD_ARG;
    cj::ZseLds* L = new_lds();
    const long long r = cj::sim_run([&] { cj::zse_build_table(L, t); return (long long)cj::zse_default_log(t); });
    if (r >= 0) {
        memcpy(st, L->st + cj::zse_st_at(t), sizeof(uint16_t) << r);
        memcpy(dnb, L->dnb + 64u * t, 256);
        memcpy(dfs, L->dfs + 64u * t, 256);
    }
    free(L);
    return r;
}

// the normaliser, the NCount writer and the table builder alone (zstd_fse_enc.h, as the kernel's lanes call them): hist[0, nsym) of
// `total` symbols at the accuracy zsf_pick_log chooses below maxlog — norm (64), the description (nc, 96 bytes; *ncb its length), the
// states (512) and deltaNbBits / deltaFindState (64 each).  Returns the log
extern "C" long long sim_zsf_table(const unsigned int* hist, unsigned int nsym, unsigned int maxlog, unsigned int total, short* norm, unsigned char* nc,
                                   unsigned int* ncb, unsigned short* st, unsigned int* dnb, int* dfs) {
    if (nsym == 0u || nsym > 64u || maxlog > 9u) return CJ_E_BAD_ARG;
    uint8_t cell[512];
    uint32_t cumul[64], used = 0, top = 0;
    for (uint32_t s = 0; s < nsym; s++) if (hist[s]) { used++; top = s; }
    const uint32_t log = zsf_pick_log(maxlog, used, total);
    zsf_normalise(hist, top + 1u, total, log, norm);
    *ncb = zsf_ncount(norm, top + 1u, log, nc, 96u);
    zsf_table(norm, top + 1u, log, st, dnb, dfs, cell, cumul);
    return log;
}
// the Huffman weights' FSE form alone: wt[0, n) into out (224 bytes); its length or 0
extern "C" unsigned int sim_zsf_weights(const unsigned char* wt, unsigned int n, unsigned char* out) {
    uint32_t hist[16], dnb[64], cumul[64];
    int32_t dfs[64];
    int16_t norm[16];
    uint16_t st[64];
    uint8_t cell[64];
    return zsf_weights(wt, n, out, 224u, hist, norm, st, dnb, dfs, cell, cumul);
}

extern "C" unsigned long long sim_zse_bound(unsigned long long n, unsigned int flags) { return cj::zse_bound(n, flags); }

#ifdef SIM_MAIN
// per case u32 flags, n, cap, in_mis, out_mis | i64 expected result | input | expected frame (result > 0)
int main(int argc, char** argv) {
    return cj::sim_cases_main(argc, argv, 5, [](FILE* f, const uint32_t* h, int64_t want, long long& got) {
        const size_t nexp = want > 0 ? (size_t)want : 0;
        cj::SimBlock in(f, h[1], h[3]), exp(f, nexp), out(nullptr, h[2], h[4]);
        if (!in.ok || !exp.ok) return 2;
        got = sim_zstd_encode(h[0], in.p, h[1], out.p, h[2], nullptr);
        return (int)(got != want || (nexp && memcmp(out.p, exp.p, nexp) != 0));
    });
}
#endif
