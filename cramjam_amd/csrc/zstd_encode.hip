// zstd_encode.hip — batches of inputs into Zstandard frames (cj_zstd_compress_batch_device / _host, cj_zstd_compress_bound;
// DESIGN.md §5.15), one frame per chunk.  One workgroup of two wavefronts owns a frame and walks its independent pieces of at most
// 64 KiB in order, one block a piece:
//   stage 1   enc2::Walk<RecFmt<65535>, 2> (cj_rec_encode.hpp, cj_enc2.hpp: the matcher of the LZ4, Snappy and DEFLATE encoders;
//             candidates up to the 16-bit table's lap, 65 535 back) leaves fixed-size sequence records in the workgroup's scratch slot
//   stage 2   zstd_enc_wave.hpp on the first wavefront: the literals gathered into the slot's literal area, Huffman or not by exact
//             size under a tree of direct or FSE-compressed weights, each sequence table RLE, FSE_Compressed or Predefined by cost (zstd_fse_enc.h), the FSE state chains walked once (pass A) and written in parallel (pass B), the block RLE, Compressed
//             or Raw.  The second wavefront runs XXH64 over the input meanwhile (once per frame, only with CJ_ZSTD_FLAG_CHECKSUM)
// The bytes are those of tests/hostsim/zstd_enc_model.c.  The slots are engine scratch within a fixed budget: a batch goes through
// in slices of as many frames as there are slots (cj::slot_slices).  The device call only enqueues (a call that grows the scratch
// waits for its previous user while it reallocates).
#include "cj_rec_encode.hpp"
#include "cj_codecs.hpp"

namespace cj {

__device__ __forceinline__ void rec_st32(DfeRec* slot, uint32_t i, uint32_t w, uint32_t v) { reinterpret_cast<uint32_t*>(slot)[4u * i + (w & 3u)] = v; }
__device__ __forceinline__ uint32_t lit_ld8(const uint8_t* p) { return *p; }
__device__ __forceinline__ void lit_st8(uint8_t* p, uint32_t v) { *p = (uint8_t)v; }

}  // namespace cj

#include "zstd_enc_wave.hpp"

namespace cj {

static_assert(kZseSlotRecs == kDfeSlotRecs, "RecFmt's slot-record bound");

// One workgroup per frame of the slice; slot blockIdx.x of `slots` is its own
__global__ __launch_bounds__(kRecEncThreads) void zstd_encode_kernel(BatchArgs a, uint8_t* slots, uint32_t flags) {
    typedef RecFmt<65535u> Fmt;
    typedef enc2::Walk<Fmt, 2> Matcher;
    __shared__ uint16_t ht_lds[kHashSize];
    __shared__ uint32_t scr[Matcher::kWords];
    __shared__ ZseLds lds;
    __shared__ uint32_t xacc[8];                   // XXH64's four accumulators
    __shared__ uint32_t sh[4];                     // 0 / 1 the checksum, 3 the frame still fits
    const uint32_t chunk = blockIdx.x;
    if (chunk >= a.n_chunks) return;
    const uint32_t wave = uni(threadIdx.x >> 6), lane = lane_id();
    const uint64_t n64 = a.in_len[chunk], cap64 = a.out_cap[chunk];
    if (n64 > kZseInMax) { if (threadIdx.x == 0) a.result[chunk] = CJ_E_INPUT_TOO_LARGE; return; }      // (the whole workgroup leaves)
    const uint32_t n = (uint32_t)n64, cap = (uint32_t)(cap64 < 0xFFFFFFF0ull ? cap64 : 0xFFFFFFF0ull);
    const uint8_t* in = a.in_base + a.in_off[chunk];
    uint8_t* out = a.out_base + a.out_off[chunk];
    uint8_t* myslot = slots + (uint64_t)blockIdx.x * kZseSlotBytes;
    DfeRec* slot = reinterpret_cast<DfeRec*>(myslot);
    if (threadIdx.x < 4) sh[threadIdx.x] = 0u;
    __syncthreads();

    ZseOut O = {out, cap, 0u};
    bool ok = true;
    uint32_t prev = 1u;                            // the frame's newest offset: Repeated_Offset1 starts at 1
    if (wave == 0u) ok = zse_begin(O, out, cap, n, flags);
    const uint32_t np = n == 0u ? 1u : (n + kZsePiece - 1u) / kZsePiece;
    const HashTab ht{ht_lds};
    for (uint32_t p = 0; p < np; p++) {
        const uint8_t* pin = in + (uint64_t)p * kZsePiece;
        const uint32_t pn = n - p * kZsePiece < kZsePiece ? n - p * kZsePiece : kZsePiece;
        // ---- stage 1: both wavefronts
        uint32_t nrec = 0, anchor = 0;
        if (pn >= 8u) {
            ht.clear(threadIdx.x, kRecEncThreads);
            ht.settle();
            Matcher w{enc2::uniform_gptr(pin), (enc2::gptr)enc2::uniform_gptr(reinterpret_cast<const uint8_t*>(slot)), pn, Fmt::last_start(pn),
                      Fmt::limit(pn), scr, ht, 0u, 0u, wave};
            anchor = w.run(0u);
            nrec = w.op;                                         // (the first wavefront's: it flushed the queue last)
        }
        if (wave == 0u) {
            nrec = nrec + 1u < kZseSlotRecs ? nrec : kZseSlotRecs - 2u;
            if (lane == 0u) slot[nrec] = DfeRec{anchor, pn - anchor, 0u, 0u};
            nrec += 1u;
        }
        __syncthreads();                                         // the records, whoever wrote them, are the first wavefront's to read
        // ---- stage 2: the first wavefront codes the piece, the second sums the input (once)
        if (wave == 0u) {
            if (ok) ok = zse_piece(&lds, O, pin, pn, slot, nrec, myslot + kZseRecBytes, p + 1u == np, (flags & kZseChecksum) ? 4u : 0u, prev, nullptr);
            if (lane == 0u) sh[3] = ok ? 1u : 0u;
        } else if (p == 0u && (flags & kZseChecksum)) {
            const uint64_t h = zse_xxh64(xacc, in, n);
            if (lane == 0u) sh[0] = (uint32_t)h;
        }
        __syncthreads();
        if (sh[3] == 0u) break;                                  // (the same word in both wavefronts: they leave together)
    }
    if (wave != 0u) return;
    int64_t r = CJ_E_OUT_TOO_SMALL;
    if (ok) r = zse_end(O, flags, lds_ld(&sh[0]));
    if (lane == 0u) a.result[chunk] = r;
}

}  // namespace cj

namespace {

// bytes of slots per slice at most: 1024 slots of 320 KiB — four workgroups per CU by LDS on 256 CUs; more slots
// would only be memory the engine keeps
cj::SlotBudget g_slot_budget{1024ull * cj::kZseSlotBytes};

bool args_ok(cj_zstd_format fmt, uint32_t flags) { return fmt == CJ_ZSTD_FRAMES && (flags & ~CJ_ZSTD_FLAG_CHECKSUM) == 0u; }

}  // namespace

// One turn at the engine's slots (cj::slot_slices); enqueue only.  A slice is what the device holds at once, within the budget.
// (Declared in cj_codecs.hpp: the ORC batch runs its ZSTD chunks through it.)
int cj::zstd_compress_device(cj_engine* e, uint32_t flags, const cj::BatchArgs& b, hipStream_t s) {
    constexpr auto kernel = &cj::zstd_encode_kernel;
    uint64_t limit;
    if (const int rc = cj::resident_limit<kernel>(e, cj::kRecEncThreads, limit)) return rc;
    return cj::slot_slices(e->zstd_enc_slots, e->d_zstd_enc_slots, cj::kZseSlotBytes, g_slot_budget.load(), limit, b, s, [&](const cj::BatchArgs& a, uint8_t* slots) {
        hipLaunchKernelGGL(kernel, dim3(a.n_chunks), dim3(cj::kRecEncThreads), 0, s, a, slots, flags);
    });
}

extern "C" {

size_t cj_zstd_compress_bound(size_t n, uint32_t flags) {
    if ((flags & ~CJ_ZSTD_FLAG_CHECKSUM) != 0u || n > cj::kZseInMax) return 0;
    return (size_t)cj::zse_bound(n, flags);
}

int cj_zstd_compress_batch_device(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                                  const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result,
                                  void* hip_stream) {
    if (!args_ok(fmt, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result);
        return cj::zstd_compress_device(e, flags, a, s);
    });
}

int cj_zstd_compress_batch_host(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                                uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!args_ok(fmt, flags)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, d_in, d_out, d);
        return cj::zstd_compress_device(e, flags, a, s);
    });
}

// tests: the bytes of slots per slice of a Zstandard compress batch (0 = the default); returns the previous value
uint64_t cj_debug_zstd_enc_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
