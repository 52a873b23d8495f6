// blosc_filters.hip — Blosc's byte shuffle and bitshuffle, both directions, over a LIST of blocks: one launch serves every block of
// every chunk of a batch, each with its own typesize (blosc_batch.hip).  A block of n = bytes / typesize elements is the byte matrix
// plain[n][typesize]; its shuffled image is the transposed matrix shuffled[typesize][n], bitshuffle additionally turns every 8 bytes
// of a row into 8 bit planes n / 8 bytes apart.  One workgroup moves one tile of E elements (E x typesize <= 16 KiB) through LDS:
//   unfilter  rows of the shuffled image -> LDS rows (bit planes are turned back on the way in) -> the plain bytes, whole dwords
//   filter    the plain bytes -> LDS as they lie -> rows of the shuffled image, whole dwords (bit planes: one byte per plane)
// so both sides of HBM see contiguous runs.  The bytes behind the last whole element are copied, and a block whose mode is kBloscCopy
// (no filter, typesize 1, bitshuffle's "element count not a multiple of 8" rule: blosc_block_mode) is copied as it is.
// Pointers may have any alignment (gfx950 runs in unaligned-access mode); nothing outside [src, src + bytes) is read, nothing
// outside [dst, dst + bytes) written.
#include "blosc_filters.hpp"

namespace cj {

namespace {

constexpr uint32_t kFilterThreads = 256;
constexpr uint32_t kRowPad = 8;                // LDS row stride E + 8 bytes: rows 4 apart (typesize 8: lanes l, l + 1) land 8+ banks apart
constexpr uint32_t kLdsBytes = 18432;          // typesize 255: 255 rows of 64 + 8 bytes

__device__ __forceinline__ void st32u(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// the filter direction keeps the plain bytes as they lie, one dword skipped every 128 bytes: the strided byte reads of a row
// (typesize 2 / 4 / 8 / 16: lanes 8 / 16 / 32 / 64 bytes apart) then fall on 32 different banks
__device__ __forceinline__ uint32_t swz(uint32_t a) { return a + ((a >> 7) << 2); }

__device__ __forceinline__ void tile_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const uint32_t t = threadIdx.x;
    const uint32_t n16 = n & ~15u;
    for (uint32_t k = 16u * t; k < n16; k += 16u * kFilterThreads) {
        uint4 v;
        __builtin_memcpy(&v, src + k, 16);
        __builtin_memcpy(dst + k, &v, 16);
    }
    if (t < n - n16) dst[n16 + t] = src[n16 + t];
}

// TS: the typesize as a constant (2, 4, 8, 16: shifts instead of divisions), 0 = read it from T
template <uint32_t TS>
__device__ __forceinline__ void unfilter_tile(uint8_t* lds, const BloscBlockRow& R, uint32_t T, uint32_t tile) {
    if (TS) T = TS;
    const uint32_t t = threadIdx.x;
    const uint32_t n = R.bytes / T, E = blosc_tile_elems(T), lgE = 31u - __builtin_clz(E), stride = E + kRowPad;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(R.src);
    uint8_t* dst = reinterpret_cast<uint8_t*>(R.dst);
    const uint32_t i0 = tile * E;
    if (tile == 0) {                                        // what lies behind the last whole element
        const uint32_t tail = R.bytes - n * T;
        if (t < tail) dst[n * T + t] = src[n * T + t];
    }
    if (i0 >= n) return;
    const uint32_t Ec = n - i0 < E ? n - i0 : E;
    if (R.mode == kBloscByte) {
        const uint32_t items = T << (lgE - 2);
        for (uint32_t idx = t; idx < items; idx += kFilterThreads) {
            const uint32_t j = idx >> (lgE - 2), i = (idx & ((E >> 2) - 1u)) << 2;
            if (i >= Ec) continue;
            const uint8_t* p = src + (uint64_t)j * n + i0 + i;
            uint32_t v = 0;
            if (i + 4 <= Ec) v = ld32u(p);
            else for (uint32_t b = 0; i + b < Ec; b++) v |= (uint32_t)p[b] << (8 * b);
            *reinterpret_cast<uint32_t*>(lds + j * stride + i) = v;
        }
    } else {                                                // bit planes: n is a multiple of 8, so are i0 and Ec
        const uint32_t n8 = n >> 3, m_end = (i0 + Ec) >> 3;
        const uint32_t items = T << (lgE - 5);
        for (uint32_t idx = t; idx < items; idx += kFilterThreads) {
            const uint32_t j = idx >> (lgE - 5), c = idx & ((E >> 5) - 1u);
            const uint32_t m0 = (i0 >> 3) + 4 * c;
            if (m0 >= m_end) continue;
            const uint32_t g = m_end - m0 < 4 ? m_end - m0 : 4;
            uint32_t w[8];
#pragma unroll
            for (uint32_t p = 0; p < 8; p++) {
                const uint8_t* q = src + (uint64_t)j * n + (uint64_t)p * n8 + m0;
                uint32_t v = 0;
                if (g == 4) v = ld32u(q);
                else for (uint32_t b = 0; b < g; b++) v |= (uint32_t)q[b] << (8 * b);
                w[p] = v;
            }
            for (uint32_t q = 0; q < g; q++) {
                uint64_t x = 0;
#pragma unroll
                for (uint32_t p = 0; p < 8; p++) x |= (uint64_t)((w[p] >> (8 * q)) & 0xffu) << (8 * p);
                *reinterpret_cast<uint64_t*>(lds + j * stride + 32 * c + 8 * q) = blosc_tr8(x);
            }
        }
    }
    __syncthreads();
    uint8_t* out = dst + (uint64_t)i0 * T;
    const uint32_t total = Ec * T, nd = total >> 2;
    for (uint32_t k = t; k < nd; k += kFilterThreads) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t pos = 4 * k + b, i = pos / T, j = pos - i * T;
            v |= (uint32_t)lds[j * stride + i] << (8 * b);
        }
        st32u(out + 4 * k, v);
    }
    if (t < (total & 3u)) {
        const uint32_t pos = 4 * nd + t, i = pos / T, j = pos - i * T;
        out[pos] = lds[j * stride + i];
    }
}

template <uint32_t TS>
__device__ __forceinline__ void filter_tile(uint8_t* lds, const BloscBlockRow& R, uint32_t T, uint32_t tile) {
    if (TS) T = TS;
    const uint32_t t = threadIdx.x;
    const uint32_t n = R.bytes / T, E = blosc_tile_elems(T), lgE = 31u - __builtin_clz(E);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(R.src);
    uint8_t* dst = reinterpret_cast<uint8_t*>(R.dst);
    const uint32_t i0 = tile * E;
    if (tile == 0) {
        const uint32_t tail = R.bytes - n * T;
        if (t < tail) dst[n * T + t] = src[n * T + t];
    }
    if (i0 >= n) return;
    const uint32_t Ec = n - i0 < E ? n - i0 : E;
    const uint8_t* in = src + (uint64_t)i0 * T;
    const uint32_t total = Ec * T, nd = total >> 2;
    for (uint32_t k = t; k < nd; k += kFilterThreads) *reinterpret_cast<uint32_t*>(lds + swz(4 * k)) = ld32u(in + 4 * k);
    if (t < (total & 3u)) lds[swz(4 * nd + t)] = in[4 * nd + t];
    __syncthreads();
    if (R.mode == kBloscByte) {
        const uint32_t items = T << (lgE - 2);
        for (uint32_t idx = t; idx < items; idx += kFilterThreads) {
            const uint32_t j = idx >> (lgE - 2), i = (idx & ((E >> 2) - 1u)) << 2;
            if (i >= Ec) continue;
            uint8_t* p = dst + (uint64_t)j * n + i0 + i;
            if (i + 4 <= Ec) {
                uint32_t v = 0;
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) v |= (uint32_t)lds[swz((i + b) * T + j)] << (8 * b);
                st32u(p, v);
            } else {
                for (uint32_t b = 0; i + b < Ec; b++) p[b] = lds[swz((i + b) * T + j)];
            }
        }
    } else {
        const uint32_t n8 = n >> 3;
        const uint32_t items = T << (lgE - 3);
        for (uint32_t idx = t; idx < items; idx += kFilterThreads) {
            const uint32_t j = idx >> (lgE - 3), m = idx & ((E >> 3) - 1u);
            if (8 * m >= Ec) continue;
            uint64_t x = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) x |= (uint64_t)lds[swz((8 * m + k) * T + j)] << (8 * k);
            const uint64_t y = blosc_tr8(x);
            uint8_t* p = dst + (uint64_t)j * n + (i0 >> 3) + m;
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) p[(uint64_t)q * n8] = (uint8_t)(y >> (8 * q));
        }
    }
}

// one workgroup per (block row, tile); gate: the chunks' results (a block of a chunk that failed is not touched), or nullptr
template <bool FWD>
__global__ __launch_bounds__(kFilterThreads) void blosc_filter_kernel(const BloscBlockRow* rows, uint32_t tiles_max, const int64_t* gate) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    const uint32_t row = blockIdx.x / tiles_max, tile = blockIdx.x - row * tiles_max;
    const BloscBlockRow R = rows[row];
    if (gate != nullptr && gate[R.chunk] < 0) return;
    const uint32_t T = R.typesize;
    if (R.mode == kBloscCopy) {
        const uint64_t at = (uint64_t)tile * kBloscTileBytes;
        if (at < R.bytes) {
            const uint32_t len = R.bytes - at < kBloscTileBytes ? (uint32_t)(R.bytes - at) : kBloscTileBytes;
            tile_copy(reinterpret_cast<uint8_t*>(R.dst) + at, reinterpret_cast<const uint8_t*>(R.src) + at, len);
        }
        return;
    }
    if (FWD) {
        switch (T) {
            case 2: filter_tile<2>(lds, R, T, tile); break;
            case 4: filter_tile<4>(lds, R, T, tile); break;
            case 8: filter_tile<8>(lds, R, T, tile); break;
            case 16: filter_tile<16>(lds, R, T, tile); break;
            default: filter_tile<0>(lds, R, T, tile);
        }
    } else {
        switch (T) {
            case 2: unfilter_tile<2>(lds, R, T, tile); break;
            case 4: unfilter_tile<4>(lds, R, T, tile); break;
            case 8: unfilter_tile<8>(lds, R, T, tile); break;
            case 16: unfilter_tile<16>(lds, R, T, tile); break;
            default: unfilter_tile<0>(lds, R, T, tile);
        }
    }
}

}  // namespace

void launch_blosc_filter(const BloscBlockRow* rows, size_t n_rows, uint32_t tiles_max, bool forward, const int64_t* gate, hipStream_t s) {
    if (n_rows == 0) return;
    if (tiles_max == 0) tiles_max = 1;
    const size_t per_launch = std::max<size_t>(1, (size_t)(1u << 30) / tiles_max);      // (grids of at most 2^30 workgroups)
    for (size_t r0 = 0; r0 < n_rows; r0 += per_launch) {
        const size_t k = std::min(per_launch, n_rows - r0);
        const dim3 grid((uint32_t)(k * tiles_max)), block(kFilterThreads);
        if (forward) hipLaunchKernelGGL(blosc_filter_kernel<true>, grid, block, 0, s, rows + r0, tiles_max, gate);
        else hipLaunchKernelGGL(blosc_filter_kernel<false>, grid, block, 0, s, rows + r0, tiles_max, gate);
    }
}

}  // namespace cj

extern "C" {

// debug aid (tests, tests/perf/blosc_rates.py): n_blocks blocks of `bytes` bytes, `stride` apart, from d_src to d_dst through the filter
// kernels (filter: 0 none, 1 byte shuffle, 2 bitshuffle, by a chunk's rules for that block size; 3: the yardstick, one device-to-device
// hipMemcpyAsync of the same span), on the engine's stream, synchronously.  ms (optional): HIP events around the launch alone.
int cj_debug_blosc_filter(cj_engine* e, int forward, uint32_t filter, uint32_t typesize, const uint8_t* d_src, uint8_t* d_dst,
                          uint64_t bytes, uint64_t stride, size_t n_blocks, double* ms) {
    if (!e || filter > 3 || typesize == 0 || typesize > 255 || bytes > cj::kBloscMaxBytes || n_blocks > 0x7FFFFFFFull) return CJ_E_BAD_ARG;
    if (ms) *ms = 0.0;
    if (n_blocks == 0) return 0;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    const uint32_t flags = filter == 1 ? cj::kBloscShuffle : filter == 2 ? cj::kBloscBitshuffle : 0u;
    std::vector<cj::BloscBlockRow> rows(n_blocks);
    for (size_t i = 0; i < n_blocks; i++)
        rows[i] = { (uint64_t)(uintptr_t)(d_src + i * stride), (uint64_t)(uintptr_t)(d_dst + i * stride), (uint32_t)bytes, typesize,
                    cj::blosc_block_mode(flags, typesize, (uint32_t)bytes), 0u };
    void* d_rows = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    HIP_TRY(hipMalloc(&d_rows, n_blocks * sizeof(cj::BloscBlockRow)), CJ_E_OOM);
    bool ok = cj::hip_ok(hipMemcpyAsync(d_rows, rows.data(), n_blocks * sizeof(cj::BloscBlockRow), hipMemcpyHostToDevice, e->stream), "hipMemcpyAsync");
    if (ok && ms) ok = cj::hip_ok(hipEventCreate(&t0), "hipEventCreate") && cj::hip_ok(hipEventCreate(&t1), "hipEventCreate") && cj::hip_ok(hipEventRecord(t0, e->stream), "hipEventRecord");
    if (ok) {
        if (filter == 3) ok = cj::hip_ok(hipMemcpyAsync(d_dst, d_src, (n_blocks - 1) * stride + bytes, hipMemcpyDeviceToDevice, e->stream), "hipMemcpyAsync");
        else cj::launch_blosc_filter((const cj::BloscBlockRow*)d_rows, n_blocks, cj::blosc_tiles(typesize, (uint32_t)bytes), forward != 0, nullptr, e->stream);
        ok = ok && cj::hip_ok(hipGetLastError(), "blosc_filter_kernel");
    }
    if (ok && ms) ok = cj::hip_ok(hipEventRecord(t1, e->stream), "hipEventRecord");
    ok = cj::hip_ok(hipStreamSynchronize(e->stream), "hipStreamSynchronize") && ok;
    if (ok && ms) { float f = 0; ok = cj::hip_ok(hipEventElapsedTime(&f, t0, t1), "hipEventElapsedTime"); *ms = f; }
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    (void)hipFree(d_rows);
    return ok ? 0 : CJ_E_NO_DEVICE;
}

}  // extern "C"
