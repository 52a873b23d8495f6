// parquet_batch.hip — batches of Parquet column chunks, decode only (cj_parquet_batch_device / _host, cj_parquet_sizes_device / _host,
// cj_parquet_pages_device / _host).  A chunk is a run of pages, each a Thrift compact PageHeader and its bytes — the
// codec's output for the page, or for the values behind a V2 page's levels —, so every page of every chunk is one entry of a batch the
// engine already runs: Snappy raw and raw LZ4 blocks (cj::launch), gzip members (deflate.hip), Zstandard frames (zstd.hip) are the inner
// kernels, unchanged.  This file is the container around them, in the shell of cj_container.hpp (the count pass, the one read-back, the
// row scan).  Parquet's own: the page walk (parquet_grammar.hpp, one lane per chunk, in both passes), the page rows — the headers state
// every decoded size, so the rows pass lays the pages out as it goes and no codec walks a page twice —, the page CRCs (one wavefront per
// page) and the page-order verdict (one wavefront per chunk).
// The size query and the pages query are the walk alone and only enqueue.  A decode takes one turn at the engine's container scratch and
// waits for the stream once, for the chunks' page counts and largest page.
#include "cj_codecs.hpp"
#include "cj_container.hpp"
#include "crc32_lanes.hpp"
#include "parquet_grammar.hpp"

namespace cj {

namespace {
__device__ const Crc32Tables d_pq_crc32_tables = make_crc32_tables();
}

// The per-page rows: the codec's batch (in_base = the chunks, out_base = the callers' slots: the values sections; a page the codec does
// not see has the stored-stream convention's row, in_len = out_cap = 0, result not looked at), the copy_segments rows (V2 levels; the
// whole payload of a page that is copied), the checksummed bytes and the page's word.
struct PqRows : CopyRows {
    uint64_t *ck_off, *ck_len;              // the payload, from in_base
    uint64_t* word;                         // the stated crc | kPq* bits << 32
};
constexpr size_t kPqRowWords = kCopyRowWords + 3;      // u64 rows per page
constexpr uint64_t kPqCoded = 1ull << 32, kPqHasCrc = 1ull << 33, kPqCrcBad = 1ull << 34;
inline PqRows pq_rows(uint64_t* base, size_t nb) {
    PqRows r;
    static_cast<CopyRows&>(r) = copy_rows(base, nb);
    r.ck_off = r.cp_len + nb; r.ck_len = r.cp_len + 2 * nb; r.word = r.cp_len + 3 * nb;
    return r;
}

// Pass 1, and alone the size query (st == nullptr: result[i] = the pages' sum or the walk's error; out_cap is not read).  Until the
// host's scan row0 holds the largest decoded page of the chunk.
__global__ __launch_bounds__(kBlockThreads) void pq_count_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                 const uint64_t* out_cap, StreamRow* st, int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t total = 0, np = 0, largest = 0;
    int64_t err = pq_walk(in_base + in_off[i], (size_t)in_len[i], [&](const PqPage& pg) {
        const uint32_t d = pg.decoded();
        np++; total += d; largest = d > largest ? d : largest;
    });
    if (st == nullptr) { result[i] = err ? err : (int64_t)total; return; }
    if (err == 0 && total > out_cap[i]) err = CJ_E_OUT_TOO_SMALL;
    st[i] = StreamRow{largest, total, err, err ? 0 : np};
}

// Pass 2: the same walk writes one row per page, the page's bytes of the caller's slot behind the pages before it.  The rows were
// counted from the same bytes; should they have changed since, a page the count does not cover or whose bytes would pass the verified
// sum gets no room, and a row the walk no longer reaches is an empty one.
__global__ __launch_bounds__(kBlockThreads) void pq_rows_kernel(uint32_t n, int codec, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                const uint64_t* out_off, const StreamRow* st, PqRows r) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const StreamRow f = st[i];
    if (f.count == 0) return;
    uint64_t k = 0, run = 0;
    const auto empty = [&](uint64_t g) {
        r.b.in_off[g] = in_off[i]; r.b.in_len[g] = 0; r.b.out_off[g] = out_off[i]; r.b.out_cap[g] = 0; r.b.result[g] = 0;
        r.cp_src[g] = 0; r.cp_dst[g] = out_off[i]; r.cp_len[g] = 0; r.ck_off[g] = in_off[i]; r.ck_len[g] = 0; r.word[g] = 0;
    };
    pq_walk(in_base + in_off[i], (size_t)in_len[i], [&](const PqPage& pg) {
        const uint32_t d = pg.decoded();
        if (k >= f.count || run + d > f.total) return;
        const uint64_t g = f.row0 + k, at = in_off[i] + pg.payload, to = out_off[i] + run;
        empty(g);
        if (!pg.skipped()) {
            const bool coded = pg.coded(codec);
            const uint32_t lv = pg.levels(), vin = (uint32_t)pg.csize - lv, vout = (uint32_t)pg.usize - lv;
            // a copied page is not held to its stated size: what both sizes cover is copied
            const uint32_t cp = coded ? lv : ((uint32_t)pg.csize < (uint32_t)pg.usize ? (uint32_t)pg.csize : (uint32_t)pg.usize);
            r.cp_src[g] = (uint64_t)(uintptr_t)(in_base + at); r.cp_dst[g] = to; r.cp_len[g] = cp;
            uint64_t w = pg.crc;
            if (coded && (vin | vout) != 0u) {                  // (0 bytes that state 0 bytes: accepted without asking the codec)
                r.b.in_off[g] = at + lv; r.b.in_len[g] = vin; r.b.out_off[g] = to + lv; r.b.out_cap[g] = vout;
                w |= kPqCoded;
            }
            if (pg.has_crc) { w |= kPqHasCrc; r.ck_off[g] = at; r.ck_len[g] = (uint32_t)pg.csize; }
            r.word[g] = w;
        }
        k++; run += d;
    });
    for (; k < f.count; k++) empty(f.row0 + k);
}

// One wavefront per page that carries a CRC: the CRC-32 of the payload as it lies in the chunk; a mismatch sets kPqCrcBad in its word
__global__ __launch_bounds__(kBlockThreads) void pq_crc_kernel(uint32_t nb, const uint8_t* in_base, PqRows r) {
    __shared__ uint32_t adv[1024];
    for (uint32_t i = threadIdx.x; i < 1024u; i += kBlockThreads) adv[i] = (&d_pq_crc32_tables.adv256[0][0])[i];
    __syncthreads();
    const uint32_t g = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (g >= nb) return;
    const uint64_t w = r.word[g];
    if (!(w & kPqHasCrc)) return;
    uint32_t c = crc32_lane(in_base + r.ck_off[g], (uint32_t)r.ck_len[g], lane_id(), adv, d_pq_crc32_tables.xpow8, [](const uint8_t* p) { return ld32u(p); });
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) c ^= __shfl_xor(c, sh, 64);
    if (lane_id() == 0 && ~c != (uint32_t)w) r.word[g] = w | kPqCrcBad;
}

// One wavefront per chunk: the walk's error or the capacity's first, then the first page in page order with a code (the lanes stride
// over the pages, a wave-wide minimum finds it) — the CRC mismatch, else the decoder's code, else CJ_E_PARQUET_SIZE where the codec
// ended well short of the stated size.
__global__ __launch_bounds__(kBlockThreads) void pq_verdict_kernel(uint32_t n, const StreamRow* st, PqRows r, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const StreamRow f = st[i];
    int64_t res = f.err ? f.err : (int64_t)f.total;
    if (f.err == 0 && f.count) {
        const auto code = [&](uint64_t k) -> int64_t {
            const uint64_t g = f.row0 + k, w = r.word[g];
            if (w & kPqCrcBad) return CJ_E_PARQUET_CRC;
            if (!(w & kPqCoded) || r.b.result[g] == (int64_t)r.b.out_cap[g]) return 0;
            return r.b.result[g] < 0 ? r.b.result[g] : (int64_t)CJ_E_PARQUET_SIZE;
        };
        const unsigned long long first = first_failing_row(f.count, [&](uint64_t k) { return code(k) != 0; });
        if (first != ~0ull) res = code(first);
    }
    if (lane_id() == 0) result[i] = res;
}

// The pages query, one lane per chunk: the page count, or the eight words of every page at tab + off_unit * off[i] bytes when that has
// room for them (cap[i] / cap_div rows).  result[i] = res_unit * the page count, or the code; a refused chunk writes nothing.
__global__ __launch_bounds__(kBlockThreads) void pq_pages_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* tab,
                                                                 const uint64_t* off, const uint64_t* cap, uint32_t off_unit, uint32_t cap_div, uint32_t res_unit,
                                                                 int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t* in = in_base + in_off[i];
    uint64_t np = 0;
    const int64_t err = pq_walk(in, (size_t)in_len[i], [&](const PqPage&) { np++; });
    if (err != 0) { result[i] = err; return; }
    if (tab != nullptr) {
        if (np > cap[i] / cap_div) { result[i] = CJ_E_OUT_TOO_SMALL; return; }
        int64_t* rows = reinterpret_cast<int64_t*>(tab + (uint64_t)off_unit * off[i]);
        uint64_t k = 0, run = 0;
        pq_walk(in, (size_t)in_len[i], [&](const PqPage& pg) {
            if (k < np) pg.words(run, rows + kPqPageWords * k);
            k++; run += pg.decoded();
        });
    }
    result[i] = (int64_t)(np * res_unit);
}

}  // namespace cj

namespace {

// enqueue only: pass 1 with the results straight into the caller's row
int pq_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s) {
    hipLaunchKernelGGL(cj::pq_count_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, nullptr, nullptr, result);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

// enqueue only
int pq_pages(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* tab, const uint64_t* off, const uint64_t* cap,
             uint32_t off_unit, uint32_t cap_div, uint32_t res_unit, int64_t* result, hipStream_t s) {
    hipLaunchKernelGGL(cj::pq_pages_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, tab, off, cap, off_unit, cap_div,
                       res_unit, result);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

int pq_decode(cj_engine* e, int codec, bool verify, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
              const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch, held across the call's one wait (cj_container.hpp)
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    cj::StreamTable t;
    uint64_t largest = 0;
    int rc = cj::stream_table(turn, e, n, cj::kPqRowWords, s, [&](cj::StreamRow* d_st) {
        hipLaunchKernelGGL(cj::pq_count_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, out_cap, d_st, nullptr);
    }, t, [&](const cj::StreamRow& f) { largest = std::max(largest, f.row0); });
    if (rc != 0) return rc;
    const cj::PqRows r = cj::pq_rows(t.rows, t.nb);
    if (t.nb) {
        hipLaunchKernelGGL(cj::pq_rows_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, codec, in_base, in_off, in_len, out_off, t.st, r);
        if (verify) hipLaunchKernelGGL(cj::pq_crc_kernel, cj::wave_grid(t.nb), dim3(cj::kBlockThreads), 0, s, (uint32_t)t.nb, in_base, r);
        if (codec != cj::kPqUncompressed && (rc = cj::inner_decode(e, cj::pq_inner(codec), largest, in_base, out_base, r.b, s)) != 0) return rc;
        cj::launch_copy_segments(r.cp_src, out_base, r.cp_dst, r.cp_len, nullptr, 0, (uint32_t)t.nb, s);
    }
    hipLaunchKernelGGL(cj::pq_verdict_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, t.st, r, result);
    return turn.done(s);
}

bool batch_args_ok(int what, cj_op op, uint32_t flags) { return cj::pq_codec_ok(what) && op == CJ_OP_DECOMPRESS && (flags & ~CJ_PARQUET_FLAG_VERIFY_CRC) == 0u; }
bool size_args_ok(int what, uint32_t flags) { return cj::pq_codec_ok(what) && flags == 0u; }

}  // namespace

extern "C" {

int cj_parquet_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                            const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!batch_args_ok(what, op, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return pq_decode(e, what, (flags & CJ_PARQUET_FLAG_VERIFY_CRC) != 0u, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_parquet_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                          uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!batch_args_ok(what, op, flags)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return pq_decode(e, what, (flags & CJ_PARQUET_FLAG_VERIFY_CRC) != 0u, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

int cj_parquet_sizes_device(cj_engine* e, int what, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                            int64_t* result, void* hip_stream) {
    if (!size_args_ok(what, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return pq_sizes(n_chunks, in_base, in_off, in_len, result, s);
    });
}

int cj_parquet_sizes_host(cj_engine* e, int what, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!size_args_ok(what, flags)) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return pq_sizes(n, d_in, d.in_off, d.in_len, d.result, s);
    });
}

int cj_parquet_pages_device(cj_engine* e, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* rows,
                            const uint64_t* row_off, const uint64_t* row_cap, int64_t* result, void* hip_stream) {
    if (flags != 0u || (rows != nullptr && n_chunks != 0 && (row_off == nullptr || row_cap == nullptr))) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return pq_pages(n_chunks, in_base, in_off, in_len, reinterpret_cast<uint8_t*>(rows), row_off, row_cap, 8u * (uint32_t)cj::kPqPageWords, 1u, 1u, result, s);
    });
}

int cj_parquet_pages_host(cj_engine* e, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* const* rows_ptrs,
                          const size_t* row_caps, int64_t* result) {
    if (flags != 0u || (rows_ptrs != nullptr && n != 0 && row_caps == nullptr)) return CJ_E_BAD_ARG;
    constexpr uint32_t kRow = 8u * (uint32_t)cj::kPqPageWords;             // bytes of a page's row
    if (rows_ptrs == nullptr)
        return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
            return pq_pages(n, d_in, d.in_off, d.in_len, nullptr, nullptr, nullptr, 1u, 1u, 1u, d.result, s);
        });
    // the tables are the staged outputs of a host batch: byte capacities, and results in bytes until they are back
    if (n > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    std::vector<size_t> caps(n);
    for (size_t i = 0; i < n; i++) {
        if (row_caps[i] > (size_t)0x7E000000u / kRow) return CJ_E_BAD_ARG;
        caps[i] = row_caps[i] * kRow;
    }
    const int rc = cj::host_call(e, n, in_ptrs, in_lens, reinterpret_cast<uint8_t* const*>(rows_ptrs), caps.data(), result, -1, false,
                                 [&](cj_engine*, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return pq_pages(n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, 1u, kRow, kRow, d.result, s);
    });
    if (rc != 0) return rc;
    for (size_t i = 0; i < n; i++)
        if (result[i] > 0) result[i] /= (int64_t)kRow;
    return 0;
}

}  // extern "C"
