// orc_batch.hip — batches of ORC compression streams (cj_orc_batch_device / _host, cj_orc_sizes_device / _host, cj_orc_compress_bound;
// DESIGN.md §5.17): the framing of every data stream, index stream and footer of an ORC file with compression != NONE.  A stream is
// chunks behind 3-byte headers, each the codec's output for at most block_size raw bytes or those bytes as they are, so every chunk
// of every stream is one entry of a batch the engine already runs: raw DEFLATE (deflate.hip), Snappy raw and raw LZ4 blocks
// (cj::launch), Zstandard frames (zstd.hip), and their encoders, are the inner kernels, unchanged.  This file is the container around
// them, bgzf_batch.hip's mapping: the hop walk (orc_grammar.hpp, one lane per stream, two passes around one read-back of the chunk
// counts), the chunk rows, the codec's size query over them — ORC states no decoded length —, the layout of the chunks in the callers'
// slots and the stream-order verdict (one wavefront per stream each), and for the encoder the layout (one wavefront per stream) and
// the assembly (one wavefront per chunk).
// NOT enqueue-only, the size query included: every call takes one turn at the engine's container scratch and waits for the stream
// once (decode, sizes: for the streams' chunk counts; compress: for the buffers' lengths and capacities).
#include "blosc_filters.hpp"      // (cj_stage.hpp; declares the codecs' launchers)
#include "orc_grammar.hpp"

namespace cj {

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
// One row per stream.  row0 comes from the host's scan of the first pass; err and total are the layout kernel's in the end.
struct OrcStream {
    uint64_t row0, total;      // first chunk row; the decoded length
    int64_t err;               // the walk's error; then the layout's: a chunk's size error, CJ_E_ORC_BLOCK, CJ_E_OUT_TOO_SMALL
    uint64_t nchunk;           // chunks of a stream the walk accepts (0 with a walk error: such a stream has no rows)
};
// The per-chunk rows: the codec's batch (in_base = the streams, out_base = the callers' slots) and the copy_segments rows of the original
// chunks.  cp_src != 0 marks an original chunk: its codec row is the stored-stream convention's (in_len = out_cap = 0, result not looked at).
struct OrcRows {
    BatchRows b;
    uint64_t *cp_src, *cp_dst, *cp_len;
};
constexpr size_t kOrcRowWords = 8;          // u64 rows per chunk
inline OrcRows orc_rows(uint64_t* base, size_t nb) {
    OrcRows r;
    r.b = batch_rows(base, nb);
    r.cp_src = r.b.end; r.cp_dst = r.b.end + nb; r.cp_len = r.b.end + 2 * nb;
    return r;
}

// Pass 1: the chunk count and the walk's error
__global__ __launch_bounds__(kBlockThreads) void orc_count_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                  OrcStream* st) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t nc = 0;
    const int64_t err = orc_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t, uint32_t, bool) { nc++; });
    st[i] = OrcStream{0, 0, err, err ? 0 : nc};
}

// Pass 2: the same walk writes one row per chunk; where it goes in the slot is the layout kernel's to say.  The rows were counted
// from the same bytes; should they have changed since, a chunk the count does not cover gets no row and a row the walk no longer
// reaches is an empty compressed one, which no size query accepts.
__global__ __launch_bounds__(kBlockThreads) void orc_rows_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                 const OrcStream* st, OrcRows r) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const OrcStream f = st[i];
    if (f.nchunk == 0) return;
    uint64_t k = 0;
    const auto put = [&](uint64_t g, uint64_t at, uint32_t len, bool orig) {
        r.b.in_off[g] = at; r.b.in_len[g] = orig ? 0u : len; r.b.out_off[g] = 0; r.b.out_cap[g] = 0; r.b.result[g] = 0;
        r.cp_src[g] = orig ? (uint64_t)(uintptr_t)(in_base + at) : 0u; r.cp_dst[g] = 0; r.cp_len[g] = orig ? len : 0u;
    };
    orc_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t off, uint32_t len, bool orig) {
        if (k < f.nchunk) { put(f.row0 + k, in_off[i] + off, len, orig); k++; }
    });
    for (; k < f.nchunk; k++) put(f.row0 + k, in_off[i], 0u, false);
}

__device__ __forceinline__ uint32_t orc_incl_scan(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane_id() >= (uint32_t)d) v += t;
    }
    return v;
}

// One wavefront per stream, behind the codec's size query (its answers lie in the result row): the sizes of the chunks in stream
// order, 64 a round, a wave prefix sum carried across the rounds.  The first chunk in stream order whose size is an error or above
// block_size refuses the stream (the codec's code / CJ_E_ORC_BLOCK); then a total above out_cap[i] does (CJ_E_OUT_TOO_SMALL).  A
// stream that stands gets every row's place in its slot; a refused one has all its rows emptied: it decodes and copies nothing.
// out_cap == nullptr: the size query — sizes[i] = the total or the error, no row is written.
__global__ __launch_bounds__(kBlockThreads) void orc_layout_kernel(uint32_t n, OrcStream* st, OrcRows r, uint32_t block_size, const uint64_t* out_off,
                                                                   const uint64_t* out_cap, int64_t* sizes) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const uint32_t lane = lane_id();
    const OrcStream f = st[i];
    int64_t err = f.err;
    uint64_t total = 0;
    // a chunk's size: an original's length, else the query's answer
    const auto size_of = [&](uint64_t g) { return r.cp_src[g] != 0u ? (int64_t)r.cp_len[g] : r.b.result[g]; };
    for (uint64_t b = 0; err == 0 && b < f.nchunk; b += 64u) {
        const bool in = b + lane < f.nchunk;
        const int64_t v = in ? size_of(f.row0 + b + lane) : 0;
        const int32_t code = v < 0 ? (int32_t)v : v > (int64_t)block_size ? (int32_t)CJ_E_ORC_BLOCK : 0;
        const uint64_t bad = ballot64(in && code != 0);
        if (bad) { err = (int64_t)(int32_t)rdlane((uint32_t)code, ctz64(bad)); break; }
        total += rdlane(orc_incl_scan((uint32_t)v), 63);
    }
    if (err == 0 && out_cap != nullptr && total > out_cap[i]) err = CJ_E_OUT_TOO_SMALL;
    if (lane == 0) { st[i].err = err; st[i].total = total; }
    if (out_cap == nullptr) {
        if (lane == 0) sizes[i] = err ? err : (int64_t)total;
        return;
    }
    uint64_t pos = out_off[i];
    for (uint64_t b = 0; b < f.nchunk; b += 64u) {
        const bool in = b + lane < f.nchunk;
        const uint64_t g = f.row0 + b + lane;
        if (err != 0) {
            if (in) { r.b.in_len[g] = 0; r.b.out_cap[g] = 0; r.cp_len[g] = 0; }
            continue;
        }
        const bool orig = in && r.cp_src[g] != 0u;
        const uint32_t v = in ? (uint32_t)size_of(g) : 0u;
        const uint32_t inc = orc_incl_scan(v);
        if (in) {
            if (orig) r.cp_dst[g] = pos + (inc - v);
            else { r.b.out_off[g] = pos + (inc - v); r.b.out_cap[g] = v; }
        }
        pos += rdlane(inc, 63);
    }
}

// One wavefront per stream: the walk's or the layout's error first, then the first failing chunk in stream order (the lanes stride
// over the chunk results, a wave-wide minimum finds it) — a compressed chunk whose decode did not give exactly its laid-out size: the
// decoder's code, or `short_code`, the codec's "corrupt", where it ended early without one.
__global__ __launch_bounds__(kBlockThreads) void orc_verdict_kernel(uint32_t n, const OrcStream* st, OrcRows r, int64_t short_code, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const OrcStream f = st[i];
    int64_t res = f.err ? f.err : (int64_t)f.total;
    if (f.err == 0 && f.nchunk) {
        unsigned long long first = ~0ull;
        for (uint64_t k = lane_id(); k < f.nchunk; k += 64u) {
            const uint64_t g = f.row0 + k;
            if (r.cp_src[g] == 0u && r.b.result[g] != (int64_t)r.b.out_cap[g]) { first = k; break; }
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const unsigned long long o = __shfl_xor(first, sh, 64);
            first = o < first ? o : first;
        }
        if (first != ~0ull) {
            res = r.b.result[f.row0 + first];
            if (res >= 0) res = short_code;
        }
    }
    if (lane_id() == 0) result[i] = res;
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------------
// One row per stream.  The pieces of all streams are numbered through; they go through the encoder in turns of as many as there are
// scratch slots.  A capacity below the bound is refused on the host, so nothing can fail later: chunks are assembled as their turn comes.
struct OrcEnc {
    uint64_t piece0, pos;      // first piece; bytes of the chunks before the current turn
    int64_t err;               // CJ_E_INPUT_TOO_LARGE, CJ_E_OUT_TOO_SMALL (host): such a stream has no pieces
    uint32_t npiece, pad;
};

// the streams without a piece: an empty buffer is an empty stream; a refused one its error
__global__ __launch_bounds__(kBlockThreads) void orc_empty_kernel(uint32_t n, const OrcEnc* enc, int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i < n && enc[i].npiece == 0u) result[i] = enc[i].err;
}

// the rows of pieces [t0, t0 + cnt): slot j of the scratch is piece t0 + j's, owner[j] its stream (the last one that begins at or
// before the piece: streams without pieces share their successor's piece0 and lie before it)
__global__ __launch_bounds__(kBlockThreads) void orc_piece_rows_kernel(uint64_t t0, uint32_t cnt, uint32_t n, const OrcEnc* enc, const uint64_t* in_off,
                                                                       const uint64_t* in_len, BatchRows r, uint32_t* owner, uint64_t stride, uint32_t block_size) {
    const uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x;
    if (j >= cnt) return;
    const uint64_t g = t0 + j;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (enc[mid].piece0 <= g) lo = mid + 1u; else hi = mid;
    }
    const uint32_t i = lo - 1u;                                           // (enc[0].piece0 = 0 <= g)
    const uint64_t at = (g - enc[i].piece0) * block_size, len = in_len[i];
    r.in_off[j] = in_off[i] + at;
    r.in_len[j] = len - at < block_size ? len - at : block_size;
    r.out_off[j] = (uint64_t)j * stride;
    r.out_cap[j] = stride;
    owner[j] = i;
}

// One wavefront per stream sa + w of a turn: a piece whose compressed length is not below its raw length (or whose encoder failed)
// becomes an original chunk — pick[j] = the chunk's header word; 3 + the chosen length of its chunks of this turn into their offsets
// in the stream, 64 at a time by a wave prefix sum behind what the turns before left; with the stream's last chunk its result.
__global__ __launch_bounds__(kBlockThreads) void orc_enc_layout_kernel(uint64_t t0, uint32_t cnt, uint32_t sa, uint32_t ns, OrcEnc* enc, const uint64_t* plen,
                                                                       const int64_t* mres, uint64_t* moff, uint32_t* pick, int64_t* result) {
    const uint32_t w = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (w >= ns) return;
    const uint32_t i = sa + w, lane = lane_id();
    const OrcEnc f = enc[i];
    if (f.npiece == 0u) return;
    const uint64_t end = f.piece0 + f.npiece;
    const uint64_t lo = f.piece0 > t0 ? f.piece0 : t0, hi = end < t0 + cnt ? end : t0 + cnt;
    if (lo >= hi) return;
    uint64_t pos = lo == f.piece0 ? 0u : f.pos;
    for (uint64_t b = lo; b < hi; b += 64u) {
        const uint64_t k = b + lane;
        const bool in = k < hi;
        const uint32_t raw = in ? (uint32_t)plen[k - t0] : 0u;
        const int64_t v = in ? mres[k - t0] : 0;
        const bool comp = in && v > 0 && v < (int64_t)raw;
        const uint32_t len = comp ? (uint32_t)v : raw;
        const uint32_t m = in ? kOrcHead + len : 0u;
        const uint32_t inc = orc_incl_scan(m);
        if (in) { moff[k - t0] = pos + (inc - m); pick[k - t0] = (len << 1) | (comp ? 0u : 1u); }
        pos += rdlane(inc, 63);
    }
    if (lane == 0u) {
        enc[i].pos = pos;
        if (hi == end) result[i] = (int64_t)pos;
    }
}

// One wavefront per chunk of a turn: the header, then the bytes from the slot or, an original chunk, from the input
__global__ __launch_bounds__(kBlockThreads) void orc_assemble_kernel(uint32_t cnt, const uint32_t* owner, const uint32_t* pick, const uint64_t* moff,
                                                                     const uint8_t* in_base, const uint64_t* pin_off, const uint8_t* slots, uint64_t stride,
                                                                     uint8_t* out_base, const uint64_t* out_off) {
    const uint32_t j = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (j >= cnt) return;
    const uint32_t i = uni(owner[j]), h = uni(pick[j]), l = lane_id();
    uint8_t* dst = out_base + out_off[i] + moff[j];
    if (l < kOrcHead) dst[l] = (uint8_t)(h >> (8u * l));
    wave_copy(dst + kOrcHead, (h & 1u) ? in_base + pin_off[j] : slots + (uint64_t)j * stride, h >> 1);
}

}  // namespace cj

namespace {

using cj::OrcEnc;
using cj::OrcStream;

inline size_t up16(size_t x) { return (x + 15u) & ~(size_t)15u; }
inline dim3 lane_grid(size_t n) { return dim3((uint32_t)((n + cj::kBlockThreads - 1) / cj::kBlockThreads)); }

// bytes of bound-sized chunk slots per turn of a compress batch at most: 1024 slots at the largest block size
cj::SlotBudget g_slot_budget{256ull << 20};

// a piece's bound-sized slot: what the codec's encoder may write for block_size bytes
uint64_t slot_stride(int kind, uint32_t block_size) {
    const size_t b = kind == cj::kOrcZlib ? cj_deflate_compress_bound(block_size, CJ_DEFLATE_RAW)
                   : kind == cj::kOrcSnappy ? cj_snappy_raw_max_compress_len(block_size)
                   : kind == cj::kOrcLz4 ? cj_lz4_block_compress_bound(block_size, 0)
                   : cj_zstd_compress_bound(block_size, 0);
    return up16(b);
}

// the codec's size query over the compressed rows: its answers into their result row.  Enqueue only
int sizes_rows(int kind, const uint8_t* in_base, const cj::BatchRows& r, hipStream_t s) {
    switch (kind) {
    case cj::kOrcZlib: return cj::launch_deflate_raw_sizes(r.n, in_base, r.in_off, r.in_len, r.result, s);
    case cj::kOrcSnappy: return cj::launch_block_sizes(CJ_CODEC_SNAPPY_RAW, r.n, in_base, r.in_off, r.in_len, r.result, s);
    case cj::kOrcLz4: return cj::launch_block_sizes(CJ_CODEC_LZ4_BLOCK, r.n, in_base, r.in_off, r.in_len, r.result, s);
    default: return cj::launch_zstd_sizes(r.n, in_base, r.in_off, r.in_len, r.result, s);
    }
}

// one codec launch over the compressed rows, straight into the callers' slots.  block_size is known here, the chunks' sizes only on
// the device: the engine's size classes are hints a chunk may break
int decode_rows(cj_engine* e, int kind, uint32_t block_size, const uint8_t* in_base, uint8_t* out_base, const cj::BatchRows& r, hipStream_t s) {
    cj::BatchArgs a;
    if (kind == cj::kOrcLz4 || kind == cj::kOrcSnappy) {
        const uint32_t flags = block_size <= 16384u ? CJ_FLAG_CHUNKS_LE_16K : block_size <= 32768u ? CJ_FLAG_CHUNKS_LE_32K : block_size > 65536u ? CJ_FLAG_BIG_CHUNKS : 0u;
        cj::fill_args(a, flags, in_base, out_base, r);
        return cj::launch(e, kind == cj::kOrcLz4 ? CJ_CODEC_LZ4_BLOCK : CJ_CODEC_SNAPPY_RAW, CJ_OP_DECOMPRESS, a, s);      // (takes e->scratch inside this call's e->fb turn)
    }
    cj::fill_args(a, 0, in_base, out_base, r);
    if (kind == cj::kOrcZlib) return cj::launch_deflate_raw_decode(a, s);
    return cj::launch_zstd_decode(e, a, s);                                                                                 // (takes e->zstd_slots inside it)
}

int64_t short_code(int kind) {
    return kind == cj::kOrcZlib ? CJ_E_DEFLATE_CORRUPT : kind == cj::kOrcSnappy ? CJ_E_SNAPPY_CORRUPT : kind == cj::kOrcLz4 ? CJ_E_CORRUPT : CJ_E_ZSTD_CORRUPT;
}

// out_cap == nullptr: the size query — result[i] = the sum of the chunks' sizes or the first error; nothing is decoded
int orc_decode(cj_engine* e, int kind, uint32_t block_size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
               const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch, as a BGZF batch takes it (bgzf_batch.hip): held across the call's one wait
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    const size_t tab = up16(n * sizeof(OrcStream));
    int rc;
    if ((rc = turn.reserve(e->d_fb, tab)) != 0 || (rc = turn.reserve(e->h_fb, tab)) != 0) return rc;
    OrcStream* h_st = reinterpret_cast<OrcStream*>(e->h_fb.p);
    hipLaunchKernelGGL(cj::orc_count_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, reinterpret_cast<OrcStream*>(e->d_fb.p));
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(h_st, e->d_fb.p, n * sizeof(OrcStream), hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);       // the one wait: the host sizes the chunk rows from the streams' chunk counts
    uint64_t nb = 0;
    for (size_t i = 0; i < n; i++) { h_st[i].row0 = nb; nb += h_st[i].nchunk; }
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    // d_fb: streams | chunk rows.  No data scratch: the chunks decode, and the original ones are copied, straight into the callers' slots
    if ((rc = turn.reserve(e->d_fb, tab + cj::kOrcRowWords * 8 * (size_t)nb + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    OrcStream* st = reinterpret_cast<OrcStream*>(d);
    const cj::OrcRows r = cj::orc_rows(reinterpret_cast<uint64_t*>(d + tab), (size_t)nb);
    HIP_TRY(hipMemcpyAsync(st, h_st, n * sizeof(OrcStream), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    if (nb) {
        hipLaunchKernelGGL(cj::orc_rows_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, st, r);
        if ((rc = sizes_rows(kind, in_base, r.b, s)) != 0) return rc;
    }
    hipLaunchKernelGGL(cj::orc_layout_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, st, r, block_size, out_off, out_cap, result);
    if (out_cap != nullptr) {
        if (nb) {
            if ((rc = decode_rows(e, kind, block_size, in_base, out_base, r.b, s)) != 0) return rc;
            cj::launch_copy_segments(r.cp_src, out_base, r.cp_dst, r.cp_len, nullptr, 0, (uint32_t)nb, s);
        }
        hipLaunchKernelGGL(cj::orc_verdict_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, st, r, short_code(kind), result);
    }
    return turn.done(s);
}

// the pieces of a turn through the codec's encoder into their slots.  Each takes its own turn at its scratch inside this call's
// e->fb turn (lock order: cj_engine.hpp)
int encode_rows(cj_engine* e, int kind, const uint8_t* in_base, uint8_t* slots, const cj::BatchRows& r, uint32_t cnt, hipStream_t s) {
    if (kind == cj::kOrcZstd)
        return cj_zstd_compress_batch_device(e, CJ_ZSTD_FRAMES, 0u, cnt, in_base, r.in_off, r.in_len, slots, r.out_off, r.out_cap, r.result, (void*)s);
    cj::BatchArgs a;
    cj::fill_args(a, 0, cnt, in_base, r.in_off, r.in_len, slots, r.out_off, r.out_cap, r.result);
    if (kind == cj::kOrcZlib) return cj::deflate_compress_device(e, CJ_DEFLATE_RAW, a, s);
    return cj::launch(e, kind == cj::kOrcLz4 ? CJ_CODEC_LZ4_BLOCK : CJ_CODEC_SNAPPY_RAW, CJ_OP_COMPRESS, a, s);
}

int orc_encode(cj_engine* e, int kind, uint32_t block_size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
               const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // The same scratch and the same one wait, for the buffers' lengths and capacities
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    const size_t tab = up16(n * sizeof(OrcEnc));
    int rc;
    if ((rc = turn.reserve(e->h_fb, 16 * n + tab)) != 0) return rc;
    const uint64_t* h_len = reinterpret_cast<const uint64_t*>(e->h_fb.p);
    const uint64_t* h_cap = h_len + n;
    OrcEnc* h_enc = reinterpret_cast<OrcEnc*>(e->h_fb.p + 16 * n);
    HIP_TRY(hipMemcpyAsync((void*)h_len, in_len, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync((void*)h_cap, out_cap, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    const uint64_t stride = slot_stride(kind, block_size);
    const uint64_t per = std::max<uint64_t>(1, g_slot_budget.load() / stride);      // chunks per turn
    uint64_t nb = 0;
    for (size_t i = 0; i < n; i++) {
        OrcEnc x = {};
        x.piece0 = nb;
        if (h_len[i] > 0x7E000000ull) x.err = CJ_E_INPUT_TOO_LARGE;
        else if (h_cap[i] < cj::orc_bound(h_len[i], block_size)) x.err = CJ_E_OUT_TOO_SMALL;      // decided before any store: nothing is written
        else x.npiece = (uint32_t)((h_len[i] + block_size - 1) / block_size);
        nb += x.npiece;
        h_enc[i] = x;
    }
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    const size_t m = (size_t)std::min(nb, per);
    // d_fb: streams | piece rows | chunk offsets | owners | header words | slots
    const size_t o_rows = tab, o_moff = o_rows + 5 * 8 * m, o_own = o_moff + 8 * m, o_pick = o_own + 4 * m, o_slots = up16(o_pick + 4 * m);
    if ((rc = turn.reserve(e->d_fb, o_slots + m * (size_t)stride + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    OrcEnc* enc = reinterpret_cast<OrcEnc*>(d);
    const cj::BatchRows r = cj::batch_rows(reinterpret_cast<uint64_t*>(d + o_rows), m);
    uint64_t* moff = reinterpret_cast<uint64_t*>(d + o_moff);
    uint32_t* owner = reinterpret_cast<uint32_t*>(d + o_own);
    uint32_t* pick = reinterpret_cast<uint32_t*>(d + o_pick);
    uint8_t* slots = d + o_slots;
    HIP_TRY(hipMemcpyAsync(enc, h_enc, n * sizeof(OrcEnc), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    hipLaunchKernelGGL(cj::orc_empty_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, enc, result);
    // the stream of piece g, as orc_piece_rows_kernel finds it
    const auto stream_of = [&](uint64_t g) {
        return (size_t)(std::upper_bound(h_enc, h_enc + n, g, [](uint64_t v, const OrcEnc& x) { return v < x.piece0; }) - h_enc) - 1;
    };
    for (uint64_t t0 = 0; t0 < nb; t0 += per) {
        const uint32_t cnt = (uint32_t)std::min(per, nb - t0);
        const size_t sa = stream_of(t0), sb = stream_of(t0 + cnt - 1);
        hipLaunchKernelGGL(cj::orc_piece_rows_kernel, lane_grid(cnt), dim3(cj::kBlockThreads), 0, s, t0, cnt, (uint32_t)n, enc, in_off, in_len, r, owner, stride,
                           block_size);
        if ((rc = encode_rows(e, kind, in_base, slots, r, cnt, s)) != 0) return rc;
        hipLaunchKernelGGL(cj::orc_enc_layout_kernel, cj::wave_grid(sb - sa + 1), dim3(cj::kBlockThreads), 0, s, t0, cnt, (uint32_t)sa, (uint32_t)(sb - sa + 1), enc,
                           r.in_len, r.result, moff, pick, result);
        hipLaunchKernelGGL(cj::orc_assemble_kernel, cj::wave_grid(cnt), dim3(cj::kBlockThreads), 0, s, cnt, owner, pick, moff, in_base, r.in_off, slots, stride,
                           out_base, out_off);
    }
    return turn.done(s);
}

bool size_args_ok(int what, uint32_t flags, uint32_t block_size) { return cj::orc_kind_ok(what) && flags == 0u && block_size >= 1u && block_size <= cj::kOrcBlockMax; }
bool orc_args_ok(int what, cj_op op, uint32_t flags, uint32_t block_size) {
    if (op == CJ_OP_COMPRESS) return size_args_ok(what, flags, block_size) && block_size <= cj::kOrcEncBlockMax;
    return op == CJ_OP_DECOMPRESS && size_args_ok(what, flags, block_size);
}

}  // namespace

extern "C" {

size_t cj_orc_compress_bound(size_t n, uint32_t block_size) {
    return (n > 0x7E000000ull || block_size < 1u || block_size > cj::kOrcEncBlockMax) ? 0 : (size_t)cj::orc_bound(n, block_size);
}

int cj_orc_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, uint32_t block_size, size_t n_streams, const uint8_t* in_base, const uint64_t* in_off,
                        const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!orc_args_ok(what, op, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_streams, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return (op == CJ_OP_DECOMPRESS ? orc_decode : orc_encode)(e, what, block_size, n_streams, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_orc_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, uint32_t block_size, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                      uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!orc_args_ok(what, op, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return (op == CJ_OP_DECOMPRESS ? orc_decode : orc_encode)(e, what, block_size, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

int cj_orc_sizes_device(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n_streams, const uint8_t* in_base, const uint64_t* in_off,
                        const uint64_t* in_len, int64_t* result, void* hip_stream) {
    if (!size_args_ok(what, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_streams, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return orc_decode(e, what, block_size, n_streams, in_base, in_off, in_len, nullptr, nullptr, nullptr, result, s);
    });
}

int cj_orc_sizes_host(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!size_args_ok(what, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine* e, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return orc_decode(e, what, block_size, n, d_in, d.in_off, d.in_len, nullptr, nullptr, nullptr, d.result, s);
    });
}

// tests: the bytes of chunk slots per turn of an ORC compress batch (0 = the default); returns the previous value
uint64_t cj_debug_orc_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
