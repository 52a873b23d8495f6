// lz4_dict.hip — batches of LZ4 blocks against ONE dictionary shared by every chunk of the call (cj_dict_batch_device / _host,
// cj_dict_batch_sizes_device / _host): what LZ4_loadDict + LZ4_compress_fast_continue write and
// LZ4_decompress_safe_usingDict reads.  Only the last 65 536 bytes of the dictionary count; a dictionary of length 0 is the plain call.
//   decompress   one wavefront per chunk, lz4_wave.hpp's lz4_wave_decode<true>: the plain decoder's text, a match that begins before the
//                block's start copies that part from the dictionary in global memory (at most 64 KiB, read by every wavefront: it lives in L2)
//   sizes        the size walk (lz4_size_walk.hpp) with the dictionary's length, one wavefront per chunk through the register window
//   compress     chunks of at most 65 536 bytes: `dictionary tail | chunk` staged contiguously per chunk in the engine's scratch, in
//                slices within a fixed budget, then the linked-block encoder (lz4_encode.hip, kFlagLinkedEnc) with hist[i] = the tail's
//                length: the bytes of tests/hostsim/enc2_linked_model.c with hist = dictionary
// The device calls only enqueue (a call that grows the engine's scratch waits for its previous user while it reallocates).
#include "cj_stage.hpp"
#include "lz4_lane_walk.hpp"
#include "lz4_size_walk.hpp"
#include "lz4_wave.hpp"


namespace cj {

constexpr uint32_t kDictWindow = 65536u;      // bytes of a dictionary that count (liblz4: the last 64 KiB)
constexpr uint32_t kDictChunkMax = 65536u;    // compress: the linked encoder's positions cover 64 KiB of history + 64 KiB of block

// ---- decompress: one wavefront per chunk ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads) void lz4_dict_decode_kernel(BatchArgs a, const uint8_t* dict_end, uint32_t hist) {
    const uint32_t chunk = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (chunk >= a.n_chunks) return;
    const uint8_t* in = a.in_base + a.in_off[chunk];
    uint64_t n64 = a.in_len[chunk];
    uint8_t* out = a.out_base + a.out_off[chunk];
    uint64_t cap64 = a.out_cap[chunk];
    const int64_t status = lz4_block_prologue(a.flags, in, n64, cap64);
    if (status != 0) { if (lane_id() == 0) a.result[chunk] = status; return; }
    const int64_t r = lz4_wave_decode<true>(in, (uint32_t)n64, out, (uint32_t)cap64, dict_end, hist);
    if (lane_id() == 0) a.result[chunk] = r;
}

// ---- sizes of raw blocks: one wavefront per chunk (lz4_size_wave_kernel's reader, batch_sizes.hip) ----------------------------------
__global__ __launch_bounds__(kBlockThreads) void lz4_dict_size_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                      const uint64_t* in_len, int64_t* result, uint32_t hist) {
    const uint32_t c = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (c >= n) return;
    const uint64_t n64 = in_len[c];
    if (n64 == 0 || n64 > kLz4InMax) { if (lane_id() == 0) result[c] = CJ_E_CORRUPT; return; }
    const uint8_t* in = in_base + in_off[c];
    InWindow w;
    const uint32_t mis = window_open(w, in, (uint32_t)n64);
    const int64_t r = lz4_size_walk([&](uint32_t p) { p = uni(p); w.ensure(p); return w.fetch32(p); },
                                    [&](uint32_t p, uint32_t e) { return uni(lz4_ff_run(w.base, uni(p), e)); }, mis, w.iend, hist);
    if (lane_id() == 0) result[c] = r;
}

// ---- compress: staging ----------------------------------------------------------------------------------------------------------
// Slot k of a slice = stage + k * stride: the dictionary's tail (hist bytes) and, right behind it, chunk first + k.  The rows of the
// encoder's batch over the slots: in_off = the chunk's place in its slot, out_off / out_cap = the caller's, behind the size prefix
// where one is asked for (the encoder itself runs without: with kFlagLinkedEnc it counts the history into the length it would
// store).  A chunk above kDictChunkMax is staged as an empty one; dict_finish_kernel gives it its verdict.
struct DictStage {
    const uint8_t* in_base; const uint64_t* in_off; const uint64_t* in_len;      // the caller's batch (rows of the slice's first chunk)
    const uint64_t* out_off; const uint64_t* out_cap;
    const uint8_t* dict_tail;
    uint8_t* stage;
    uint64_t *r_in_off, *r_in_len, *r_out_off, *r_out_cap;
    uint32_t* r_hist;
    uint64_t stride;
    uint32_t hist, n, prefix;
};

__device__ __forceinline__ void block_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {      // dst 16-byte aligned
    const uint32_t wide = n & ~15u;
    for (uint32_t k = threadIdx.x * 16u; k < wide; k += kBlockThreads * 16u) {
        uint4 v;
        __builtin_memcpy(&v, src + k, 16);
        *reinterpret_cast<uint4*>(dst + k) = v;
    }
    for (uint32_t k = wide + threadIdx.x; k < n; k += kBlockThreads) dst[k] = src[k];
}

__global__ __launch_bounds__(kBlockThreads) void dict_stage_kernel(DictStage g) {
    const uint32_t k = blockIdx.x;
    if (k >= g.n) return;
    const uint64_t len64 = g.in_len[k];
    const uint32_t len = len64 <= kDictChunkMax ? (uint32_t)len64 : 0u;
    uint8_t* slot = g.stage + (uint64_t)k * g.stride;
    block_copy(slot, g.dict_tail, g.hist);
    const uint32_t head = (16u - (g.hist & 15u)) & 15u;                 // bytes up to the slot's next 16-byte boundary
    const uint8_t* src = g.in_base + g.in_off[k];
    if (len <= head) {
        if (threadIdx.x < len) slot[g.hist + threadIdx.x] = src[threadIdx.x];
    } else {
        if (threadIdx.x < head) slot[g.hist + threadIdx.x] = src[threadIdx.x];
        block_copy(slot + g.hist + head, src + head, len - head);
    }
    if (threadIdx.x == 0) {
        const uint64_t cap = g.out_cap[k], pre = g.prefix ? 4u : 0u;
        g.r_in_off[k] = (uint64_t)k * g.stride + g.hist;
        g.r_in_len[k] = len;
        g.r_out_off[k] = g.out_off[k] + pre;
        g.r_out_cap[k] = cap >= pre ? cap - pre : 0u;
        g.r_hist[k] = g.hist;
    }
}

// the verdict of a chunk that is too long, and the size prefix in front of the others
__global__ __launch_bounds__(kBlockThreads) void dict_finish_kernel(uint32_t n, const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off,
                                                                    int64_t* result, uint32_t prefix) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = in_len[i];
    if (len > kDictChunkMax) { result[i] = CJ_E_INPUT_TOO_LARGE; return; }
    const int64_t r = result[i];
    if (!prefix || r < 0) return;
    uint8_t* out = out_base + out_off[i];              // (r >= 0: the encoder was given out_cap - 4 >= 0 bytes behind these four)
    for (uint32_t b = 0; b < 4u; b++) out[b] = (uint8_t)(len >> (8u * b));
    result[i] = r + 4;
}

}  // namespace cj

namespace {

cj::SlotBudget g_stage_budget{1ull << 30};      // bytes of staged slots per slice

bool args_ok(int codec, uint32_t flags, const void* dict, size_t dict_len) {
    return codec == CJ_CODEC_LZ4_BLOCK && (flags & ~CJ_FLAG_LZ4_SIZE_PREFIX) == 0u && (dict_len == 0 || dict != nullptr);
}

// One turn at the engine's staging scratch (cj::ScratchTurn)
int compress_device(cj_engine* e, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                    const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, const uint8_t* dict_tail, uint32_t hist, hipStream_t s) {
    const uint64_t stride = ((uint64_t)hist + cj::kDictChunkMax + 255u) & ~(uint64_t)255u;
    const uint64_t budget = g_stage_budget.load();
    const size_t per = (size_t)std::min<uint64_t>(n, std::max<uint64_t>(1, budget / stride));
    const size_t slots_bytes = per * stride + 256;                      // (the encoder's vector loads may pass a chunk's end by a granule)
    const size_t rows_bytes = per * (4 * 8 + 4) + 64;
    cj::ScratchTurn turn(e->dict_stage, s);
    if (turn.rc != 0 || (turn.rc = turn.reserve(e->d_dict_stage, slots_bytes + rows_bytes)) != 0) return turn.rc;
    uint8_t* stage = (uint8_t*)e->d_dict_stage.p;
    uint64_t* rows = reinterpret_cast<uint64_t*>(stage + slots_bytes);
    const uint32_t prefix = (flags & CJ_FLAG_LZ4_SIZE_PREFIX) ? 1u : 0u;
    for (size_t first = 0; first < n; first += per) {      // (the slices of the staging budget: their rows are the slots', not the caller's)
        const uint32_t k = (uint32_t)std::min(per, n - first);
        cj::DictStage g = {in_base, in_off + first, in_len + first, out_off + first, out_cap + first, dict_tail, stage,
                           rows, rows + per, rows + 2 * per, rows + 3 * per, reinterpret_cast<uint32_t*>(rows + 4 * per), stride, hist, k, prefix};
        hipLaunchKernelGGL(cj::dict_stage_kernel, dim3(k), dim3(cj::kBlockThreads), 0, s, g);
        cj::BatchArgs a;
        cj::fill_args(a, cj::kFlagLinkedEnc, k, stage, g.r_in_off, g.r_in_len, out_base, g.r_out_off, g.r_out_cap, result + first);
        a.hist = g.r_hist;
        HIP_TRY(cj::launch_lz4_encode(a, s), CJ_E_NO_DEVICE);
    }
    cj::for_slices(n, cj::grid_chunks() << 6, 0u, in_base, in_off, in_len, out_base, out_off, out_cap, result, [&](const cj::BatchArgs& a) {      // one lane per chunk
        hipLaunchKernelGGL(cj::dict_finish_kernel, dim3((a.n_chunks + cj::kBlockThreads - 1) / cj::kBlockThreads), dim3(cj::kBlockThreads), 0, s, a.n_chunks, a.in_len,
                           out_base, a.out_off, a.result, prefix);
    });
    return turn.done(s);
}

// enqueue only; dict = the whole dictionary on the device, dict_len > 0
int batch_launch(cj_engine* e, cj_op op, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                 uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, const uint8_t* dict, size_t dict_len, hipStream_t s) {
    const uint32_t hist = (uint32_t)std::min<size_t>(dict_len, cj::kDictWindow);
    const uint8_t* dict_end = dict + dict_len;
    if (op == CJ_OP_COMPRESS)
        return compress_device(e, flags, n, in_base, in_off, in_len, out_base, out_off, out_cap, result, dict_end - hist, hist, s);
    cj::for_slices(n, cj::grid_chunks(), flags, in_base, in_off, in_len, out_base, out_off, out_cap, result, [&](const cj::BatchArgs& a) {
        hipLaunchKernelGGL(cj::lz4_dict_decode_kernel, cj::wave_grid(a.n_chunks), dim3(cj::kBlockThreads), 0, s, a, dict_end, hist);
    });
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

int sizes_launch(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, size_t dict_len, hipStream_t s) {
    const uint32_t hist = (uint32_t)std::min<size_t>(dict_len, cj::kDictWindow);
    cj::for_slices(n, cj::grid_chunks(), 0u, in_base, in_off, in_len, nullptr, nullptr, nullptr, result, [&](const cj::BatchArgs& a) {
        hipLaunchKernelGGL(cj::lz4_dict_size_kernel, cj::wave_grid(a.n_chunks), dim3(cj::kBlockThreads), 0, s, a.n_chunks, a.in_base, a.in_off, a.in_len, a.result, hist);
    });
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

// the tail of a host dictionary that counts, uploaded into e->d_dict on s (e->mu held): the device pointer behind its last byte
int upload_dict(cj_engine* e, const uint8_t* dict_host, size_t dict_len, hipStream_t s, const uint8_t** d_end, size_t* kept) {
    const size_t hist = std::min<size_t>(dict_len, cj::kDictWindow);
    if (!e->d_dict.reserve(hist + 16)) return CJ_E_OOM;
    HIP_TRY(hipMemcpyAsync(e->d_dict.p, dict_host + dict_len - hist, hist, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    *d_end = (const uint8_t*)e->d_dict.p + hist;
    *kept = hist;
    return 0;
}

}  // namespace

extern "C" {

int cj_dict_batch_device(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                         const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result,
                         const uint8_t* dict_dev, size_t dict_len, void* hip_stream) {
    if (!args_ok((int)codec, flags, dict_dev, dict_len) || (op != CJ_OP_DECOMPRESS && op != CJ_OP_COMPRESS)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        if (dict_len == 0) return cj_batch_device(e, codec, op, flags, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result, hip_stream);
        return batch_launch(e, op, flags, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result, dict_dev, dict_len, s);
    });
}

int cj_dict_batch_host(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                       uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result, const uint8_t* dict_host, size_t dict_len) {
    if (!args_ok((int)codec, flags, dict_host, dict_len) || (op != CJ_OP_DECOMPRESS && op != CJ_OP_COMPRESS)) return CJ_E_BAD_ARG;
    // (a dictionary of length 0 is the plain batch, which stages for itself: the gate and the engine stay here)
    const int g = cj::batch_gate(n, {in_ptrs, in_lens, out_ptrs, out_caps, result});
    if (g != cj::kBatchGo) return g;
    if (!e && !(e = cj::default_engine())) return CJ_E_NO_DEVICE;
    if (dict_len == 0) return cj_batch_host(e, codec, op, flags, n, in_ptrs, in_lens, out_ptrs, out_caps, result);
    const int lz4_room = op == CJ_OP_COMPRESS ? ((flags & CJ_FLAG_LZ4_SIZE_PREFIX) ? 1 : 0) : -1;
    return cj::host_batch(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, lz4_room, [&](const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        const uint8_t* d_end = nullptr;
        size_t kept = 0;
        const int rc = upload_dict(e, dict_host, dict_len, s, &d_end, &kept);      // once per call
        if (rc != 0) return rc;
        return batch_launch(e, op, flags, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, d_end - kept, kept, s);
    });
}

int cj_dict_batch_sizes_device(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                               const uint64_t* in_len, int64_t* result, size_t dict_len, void* hip_stream) {
    if (!args_ok((int)codec, flags, "", dict_len)) return CJ_E_BAD_ARG;
    // the prefix answers without the stream, a dictionary of length 0 is the plain query
    if (dict_len == 0 || (flags & CJ_FLAG_LZ4_SIZE_PREFIX)) return cj_batch_sizes_device(e, codec, flags, n_chunks, in_base, in_off, in_len, result, hip_stream);
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return sizes_launch(n_chunks, in_base, in_off, in_len, result, dict_len, s);
    });
}

int cj_dict_batch_sizes_host(cj_engine* e, cj_codec codec, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result,
                             size_t dict_len) {
    if (!args_ok((int)codec, flags, "", dict_len)) return CJ_E_BAD_ARG;
    if (dict_len == 0 || (flags & CJ_FLAG_LZ4_SIZE_PREFIX)) return cj_batch_sizes_host(e, codec, flags, n, in_ptrs, in_lens, result);
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return sizes_launch(n, d_in, d.in_off, d.in_len, d.result, dict_len, s);
    });
}

// tests: the staging budget of dictionary compress in bytes (0 = the default); returns the previous value
uint64_t cj_debug_dict_stage_budget(uint64_t bytes) { return g_stage_budget.exchange(bytes); }

}  // extern "C"
