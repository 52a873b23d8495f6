// deflate_encode.hip — batches of inputs into DEFLATE streams (cj_deflate_compress_batch_device / _host, cj_deflate_compress_bound;
// DESIGN.md §5.13): raw DEFLATE, zlib streams and gzip members, one stream per chunk.  One workgroup of two wavefronts owns a stream
// and walks its independent pieces of at most 64 KiB in order:
//   stage 1   enc2::Walk<RecFmt<32768>, 2> (cj_rec_encode.hpp, cj_enc2.hpp: the matcher of the LZ4 and Snappy encoders, candidates
//             limited to 32 768 back) leaves fixed-size sequence records in the workgroup's scratch slot; the literals stay in the input
//   stage 2   deflate_enc_wave.hpp on the first wavefront: histograms, length-limited codes, the exact costs of a stored, a fixed and
//             a dynamic block, the block behind the bit position the previous one left.  The second wavefront sums the input meanwhile
//             (Adler-32 / CRC-32, once per stream)
// The bytes are those of tests/hostsim/deflate_enc_model.c.  The slots are engine scratch within a fixed budget: a batch goes through
// in slices of as many streams as there are slots (cj::slot_slices).  The device call only enqueues (a call that grows the scratch
// waits for its previous user while it reallocates).
#include "cj_rec_encode.hpp"
#include "cj_codecs.hpp"
#include "crc32_lanes.hpp"

namespace cj {

__device__ const Crc32Tables d_crc32_enc_tables = make_crc32_tables();

// One workgroup per stream of the slice; slot blockIdx.x of `slots` is its own
template <int WRAP>
__global__ __launch_bounds__(kRecEncThreads) void deflate_encode_kernel(BatchArgs a, uint8_t* slots) {
    typedef RecFmt<32768u> Fmt;
    typedef enc2::Walk<Fmt, 2> Matcher;
    __shared__ uint16_t ht_lds[kHashSize];
    __shared__ uint32_t scr[Matcher::kWords];
    __shared__ DfeLds lds;
    __shared__ uint32_t crc_adv[WRAP == kDfeGzip ? 1024 : 1];
    __shared__ uint32_t sh[8];                     // 0 / 1 Adler-32's two sums, 2 the CRC register, 3 the stream still fits
    const uint32_t chunk = blockIdx.x;
    if (chunk >= a.n_chunks) return;
    const uint32_t wave = uni(threadIdx.x >> 6), lane = lane_id();
    const uint64_t n64 = a.in_len[chunk], cap64 = a.out_cap[chunk];
    if (n64 > kDfeInMax) { if (threadIdx.x == 0) a.result[chunk] = CJ_E_INPUT_TOO_LARGE; return; }      // (the whole workgroup leaves)
    const uint32_t n = (uint32_t)n64, cap = (uint32_t)(cap64 < 0xFFFFFFF0ull ? cap64 : 0xFFFFFFF0ull);
    const uint8_t* in = a.in_base + a.in_off[chunk];
    uint8_t* out = a.out_base + a.out_off[chunk];
    DfeRec* slot = reinterpret_cast<DfeRec*>(slots + (uint64_t)blockIdx.x * kRecBytes);
    if (WRAP == kDfeGzip)
        for (uint32_t i = threadIdx.x; i < 1024u; i += kRecEncThreads) crc_adv[i] = (&d_crc32_enc_tables.adv256[0][0])[i];
    if (threadIdx.x < 8) sh[threadIdx.x] = 0u;
    __syncthreads();

    DfeOut W = {out, cap, 0u, 0u};
    bool ok = true;
    if (wave == 0u) ok = dfe_begin(&lds, W, WRAP, out, cap);
    const uint32_t np = n == 0u ? 1u : (n + kDfePiece - 1u) / kDfePiece;
    const HashTab ht{ht_lds};
    for (uint32_t p = 0; p < np; p++) {
        const uint8_t* pin = in + (uint64_t)p * kDfePiece;
        const uint32_t pn = n - p * kDfePiece < kDfePiece ? n - p * kDfePiece : kDfePiece;
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
            nrec = nrec + 1u < kDfeSlotRecs ? nrec : kDfeSlotRecs - 2u;
            if (lane == 0u) slot[nrec] = DfeRec{anchor, pn - anchor, 0u, 0u};
            nrec += 1u;
        }
        __syncthreads();                                         // the records, whoever wrote them, are the first wavefront's to read
        // ---- stage 2: the first wavefront codes the piece, the second sums the input (once)
        if (wave == 0u) {
            if (ok) ok = dfe_piece(&lds, W, pin, pn, slot, nrec, p + 1u == np, dfe_tail_bytes(WRAP), nullptr);
            if (lane == 0u) sh[3] = ok ? 1u : 0u;
        } else if (p == 0u) {
            const auto ld32 = [](const uint8_t* q) { uint32_t x; __builtin_memcpy(&x, q, 4); return x; };
            if (WRAP == kDfeZlib) {
                uint32_t s1, s2;
                adler32_lane(in, n, lane, ld32, s1, s2);
                lds_add(&sh[0], s1);
                lds_add(&sh[1], s2);
            }
            if (WRAP == kDfeGzip) lds_xor(&sh[2], crc32_lane(in, n, lane, crc_adv, d_crc32_enc_tables.xpow8, ld32));
        }
        __syncthreads();
        if (sh[3] == 0u) break;                                  // (the same word in both wavefronts: they leave together)
    }
    if (wave != 0u) return;
    int64_t r = CJ_E_OUT_TOO_SMALL;
    if (ok) {
        uint32_t sum = 0;
        if (WRAP == kDfeZlib) {
            const uint32_t s1 = (1u + lds_ld(&sh[0])) % 65521u, s2 = (n % 65521u + lds_ld(&sh[1])) % 65521u;
            sum = (s2 << 16) | s1;
        }
        if (WRAP == kDfeGzip) sum = ~lds_ld(&sh[2]);
        r = dfe_end(&lds, W, WRAP, sum, n);
    }
    if (lane == 0u) a.result[chunk] = r;
}

}  // namespace cj

namespace {

// bytes of record slots per slice at most: 1280 slots, the workgroups of the raw / zlib kernel that 256 CUs hold at
// once (five per CU by LDS) — more slots would only be memory the engine keeps
cj::SlotBudget g_slot_budget{1280ull * cj::kRecBytes};

template <int WRAP>
int compress_wrap(cj_engine* e, const cj::BatchArgs& b, hipStream_t s) {
    constexpr auto kernel = &cj::deflate_encode_kernel<WRAP>;
    uint64_t limit;
    if (const int rc = cj::resident_limit<kernel>(e, cj::kRecEncThreads, limit)) return rc;
    return cj::slot_slices(e->deflate_slots, e->d_deflate_slots, cj::kRecBytes, g_slot_budget.load(), limit, b, s, [&](const cj::BatchArgs& a, uint8_t* slots) {
        hipLaunchKernelGGL(kernel, dim3(a.n_chunks), dim3(cj::kRecEncThreads), 0, s, a, slots);
    });
}

}  // namespace

// One turn at the engine's record slots (cj::slot_slices); enqueue only.  A slice is what the device holds at once — a launch of more
// workgroups than that ends in a tail of a few of them (gzip, four per CU, on synth-v1: 25.7 GB/s in slices of 1280, 37.8 in slices of 1024) —
// within the budget.  (Declared in cj_codecs.hpp: the BGZF and ORC batches run their members and chunks through it.)
int cj::deflate_compress_device(cj_engine* e, int wrap, const cj::BatchArgs& b, hipStream_t s) {
    if (wrap == CJ_DEFLATE_RAW) return compress_wrap<cj::kDfeRaw>(e, b, s);
    if (wrap == CJ_DEFLATE_ZLIB) return compress_wrap<cj::kDfeZlib>(e, b, s);
    return compress_wrap<cj::kDfeGzip>(e, b, s);
}

extern "C" {

size_t cj_deflate_compress_bound(size_t n, cj_deflate_wrap wrap) {
    if (!cj::deflate_wrap_ok((int)wrap) || n > cj::kDfeInMax) return 0;
    return (size_t)cj::dfe_bound(n, (int)wrap);
}

int cj_deflate_compress_batch_device(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                                     const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result,
                                     void* hip_stream) {
    if (!cj::deflate_wrap_ok((int)wrap) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result);
        return cj::deflate_compress_device(e, (int)wrap, a, s);
    });
}

int cj_deflate_compress_batch_host(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                                   uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!cj::deflate_wrap_ok((int)wrap) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, d_in, d_out, d);
        return cj::deflate_compress_device(e, (int)wrap, a, s);
    });
}

// tests: the bytes of record slots per slice of a DEFLATE compress batch (0 = the default); returns the previous value
uint64_t cj_debug_deflate_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
