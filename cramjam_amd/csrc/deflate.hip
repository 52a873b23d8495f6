// deflate.hip — batches of DEFLATE streams, decode only (cj_deflate_batch_device / _host, cj_deflate_batch_sizes_device / _host;
// DESIGN.md §5.12): raw DEFLATE, zlib streams and gzip members, one stream per chunk, one wavefront per stream, workgroups of four
// wavefronts.  The decoder is deflate_wave.hpp (the same text tests/hostsim compiles for the host); this file gives it the wavefront:
// the accessors (wave_lanes.hpp), each wavefront's private tables in static LDS (9.6 KiB each; the gzip decode adds the workgroup's
// 4 KiB of CRC-32 tables), and the launches.  The size query is the same decoder with stores and checksums compiled out.
// The device calls only enqueue: no wait, no read-back, no engine scratch, no lock.
#include "wave_lanes.hpp"
#include "cj_stage.hpp"
#include "cj_codecs.hpp"
#include "deflate_wave.hpp"

namespace cj {

__device__ const Crc32Tables d_crc32_tables = make_crc32_tables();

// One wavefront per stream.  SIZE: out_base / out_off / out_cap are not read.
template <int WRAP, bool SIZE>
__global__ __launch_bounds__(kBlockThreads) void deflate_kernel(BatchArgs a) {
    __shared__ DeflateLds lds[kWavesPerBlock];
    __shared__ uint32_t crc_adv[(WRAP == CJ_DEFLATE_GZIP && !SIZE) ? 1024 : 1];
    if (WRAP == CJ_DEFLATE_GZIP && !SIZE) {                    // (before any wavefront leaves: every thread reaches this barrier)
        for (uint32_t i = threadIdx.x; i < 1024u; i += kBlockThreads) crc_adv[i] = (&d_crc32_tables.adv256[0][0])[i];
        __syncthreads();
    }
    const uint32_t wave = uni(threadIdx.x >> 6);
    const uint32_t chunk = uni(blockIdx.x * kWavesPerBlock + wave);
    if (chunk >= a.n_chunks) return;
    const uint64_t n64 = a.in_len[chunk];
    const uint64_t cap64 = SIZE ? 0u : a.out_cap[chunk];
    int64_t r;
    if (n64 > 0x7FFFFFF0ull) r = CJ_E_CORRUPT;
    else if (cap64 > kDfOutMax) r = CJ_E_PREFIX_TOO_BIG;
    else r = deflate_wave_decode<WRAP, SIZE>(a.in_base + a.in_off[chunk], (uint32_t)n64, SIZE ? nullptr : a.out_base + a.out_off[chunk], (uint32_t)cap64,
                                             &lds[wave], crc_adv, d_crc32_tables.xpow8);
    if (lane_id() == 0) a.result[chunk] = r;
}

}  // namespace

namespace {

template <int WRAP, bool SIZE>
void launch_one(const cj::BatchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((cj::deflate_kernel<WRAP, SIZE>), cj::wave_grid(a.n_chunks), dim3(cj::kBlockThreads), 0, s, a);
}

}  // namespace

// enqueue only; size: the size query (the output rows are null).  The containers' one DEFLATE launch too (cj_codecs.hpp)
int cj::launch_deflate(int wrap, bool size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                       const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    cj::for_slices(n, cj::grid_chunks(), 0u, in_base, in_off, in_len, out_base, size ? nullptr : out_off, size ? nullptr : out_cap, result, [&](const cj::BatchArgs& a) {
        switch (wrap * 2 + (size ? 1 : 0)) {
        case 0: launch_one<CJ_DEFLATE_RAW, false>(a, s); break;
        case 1: launch_one<CJ_DEFLATE_RAW, true>(a, s); break;
        case 2: launch_one<CJ_DEFLATE_ZLIB, false>(a, s); break;
        case 3: launch_one<CJ_DEFLATE_ZLIB, true>(a, s); break;
        case 4: launch_one<CJ_DEFLATE_GZIP, false>(a, s); break;
        default: launch_one<CJ_DEFLATE_GZIP, true>(a, s); break;
        }
    });
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

extern "C" {

int cj_deflate_batch_device(cj_engine* e, cj_deflate_wrap wrap, cj_op op, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                            const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!cj::deflate_wrap_ok((int)wrap) || op != CJ_OP_DECOMPRESS || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return cj::launch_deflate((int)wrap, false, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_deflate_batch_host(cj_engine* e, cj_deflate_wrap wrap, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                          uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!cj::deflate_wrap_ok((int)wrap) || op != CJ_OP_DECOMPRESS || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine*, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return cj::launch_deflate((int)wrap, false, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

int cj_deflate_batch_sizes_device(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                                  const uint64_t* in_len, int64_t* result, void* hip_stream) {
    if (!cj::deflate_wrap_ok((int)wrap) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return cj::launch_deflate((int)wrap, true, n_chunks, in_base, in_off, in_len, nullptr, nullptr, nullptr, result, s);
    });
}

int cj_deflate_batch_sizes_host(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!cj::deflate_wrap_ok((int)wrap) || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return cj::launch_deflate((int)wrap, true, n, d_in, d.in_off, d.in_len, nullptr, nullptr, nullptr, d.result, s);
    });
}

}  // extern "C"
