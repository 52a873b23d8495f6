// zstd.hip — batches of Zstandard chunks, decode only (cj_zstd_batch_device / _host, cj_zstd_batch_sizes_device / _host; DESIGN.md
// §5.14): one chunk = what one ZSTD_decompress call reads, one wavefront per chunk, workgroups of four wavefronts.  The decoder is
// zstd_wave.hpp (the same text tests/hostsim compiles for the host); this file gives it the wavefront: the accessors (wave_lanes.hpp), each wavefront's
// private tables in static LDS (10.0 KiB each), its literal slot in engine scratch and the launches.  The slots come from a fixed
// budget (cj::slot_slices on e->zstd_slots): a batch goes through in slices of as many chunks as there are slots.  The size query is
// the same decoder without stores and uses no scratch.  The device calls only enqueue (a decode that grows the slots waits for their
// previous user while it reallocates).
#include "wave_lanes.hpp"
#include "cj_stage.hpp"
#include "cj_codecs.hpp"
#include "zstd_wave.hpp"

namespace cj {

static_assert(kZsOutMax == 0x7E000000u, "the capacity limit of every decoder");

// One wavefront per chunk; slot (blockIdx.x * 4 + wave) of `slots` is its own.  SIZE: out_base / out_off / out_cap / slots are not read.
template <bool SIZE>
__global__ __launch_bounds__(kBlockThreads) void zstd_kernel(BatchArgs a, uint8_t* slots) {
    __shared__ ZstdLds lds[kWavesPerBlock];
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t chunk = uni(blockIdx.x * kWavesPerBlock + wave);
    if (chunk >= a.n_chunks) return;
    const uint64_t n64 = a.in_len[chunk];
    const uint64_t cap64 = SIZE ? 0u : a.out_cap[chunk];
    int64_t r;
    if (n64 > 0x7FFFFFF0ull) r = CJ_E_CORRUPT;
    else if (cap64 > kZsOutMax) r = CJ_E_PREFIX_TOO_BIG;
    else r = zstd_wave_decode<SIZE>(a.in_base + a.in_off[chunk], (uint32_t)n64, SIZE ? nullptr : a.out_base + a.out_off[chunk], (uint32_t)cap64,
                                    &lds[wave], SIZE ? nullptr : slots + (uint64_t)chunk * kZsSlotBytes);
    if (lane_id() == 0) a.result[chunk] = r;
}

}  // namespace cj

namespace {

// bytes of literal slots per slice at most: 4096 slots, the wavefronts that 256 CUs hold at once (four workgroups per CU by LDS)
cj::SlotBudget g_slot_budget{4096ull * cj::kZsSlotBytes};

bool fmt_ok(int fmt) { return fmt == CJ_ZSTD_FRAMES; }

}  // namespace

// the size query: enqueue only, no scratch
int cj::launch_zstd_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s) {
    cj::for_slices(n, cj::grid_chunks(), 0u, in_base, in_off, in_len, nullptr, nullptr, nullptr, result, [&](const cj::BatchArgs& a) {
        hipLaunchKernelGGL((cj::zstd_kernel<true>), cj::wave_grid(a.n_chunks), dim3(cj::kBlockThreads), 0, s, a, (uint8_t*)nullptr);
    });
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

// One turn at the engine's literal slots (cj::slot_slices); enqueue only.  A caller may hold the e->fb turn (cj::inner_decode), never
// the other way round: the lock order is written down where cj_engine declares the scratches
int cj::launch_zstd_decode(cj_engine* e, const cj::BatchArgs& b, hipStream_t s) {
    return cj::slot_slices(e->zstd_slots, e->d_zstd_slots, cj::kZsSlotBytes, g_slot_budget.load(), cj::grid_chunks(), b, s,
                           [&](const cj::BatchArgs& a, uint8_t* slots) {
        hipLaunchKernelGGL((cj::zstd_kernel<false>), cj::wave_grid(a.n_chunks), dim3(cj::kBlockThreads), 0, s, a, slots);
    });
}

extern "C" {

int cj_zstd_batch_device(cj_engine* e, cj_zstd_format fmt, cj_op op, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                         const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!fmt_ok((int)fmt) || op != CJ_OP_DECOMPRESS || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result);
        return cj::launch_zstd_decode(e, a, s);
    });
}

int cj_zstd_batch_host(cj_engine* e, cj_zstd_format fmt, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                       uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!fmt_ok((int)fmt) || op != CJ_OP_DECOMPRESS || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, d_in, d_out, d);
        return cj::launch_zstd_decode(e, a, s);
    });
}

int cj_zstd_batch_sizes_device(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                               const uint64_t* in_len, int64_t* result, void* hip_stream) {
    if (!fmt_ok((int)fmt) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return cj::launch_zstd_sizes(n_chunks, in_base, in_off, in_len, result, s);
    });
}

int cj_zstd_batch_sizes_host(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!fmt_ok((int)fmt) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return cj::launch_zstd_sizes(n, d_in, d.in_off, d.in_len, d.result, s);
    });
}

// tests: the bytes of literal slots per slice of a Zstandard decode batch (0 = the default); returns the previous value
uint64_t cj_debug_zstd_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
