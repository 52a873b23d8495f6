// orc_batch.hip — batches of ORC compression streams (cj_orc_batch_device / _host, cj_orc_sizes_device / _host, cj_orc_compress_bound;
// DESIGN.md §5.17): the framing of every data stream, index stream and footer of an ORC file with compression != NONE.  A stream is
// chunks behind 3-byte headers, each the codec's output for at most block_size raw bytes or those bytes as they are, so every chunk
// of every stream is one entry of a batch the engine already runs: raw DEFLATE (deflate.hip), Snappy raw and raw LZ4 blocks
// (cj::launch), Zstandard frames (zstd.hip), and their encoders, are the inner kernels, unchanged.  This file is the container around
// them, in the shell of cj_container.hpp (the count pass, the one read-back, the row scan; the encoder's piece turns).  ORC's own: the
// hop walk (orc_grammar.hpp, one lane per stream, in both passes), the chunk rows, the codec's size query over them — ORC states no
// decoded length —, the layout of the chunks in the callers' slots and the stream-order verdict (one wavefront per stream each), and for
// the encoder the layout (one wavefront per stream) and the assembly (one wavefront per chunk).
// NOT enqueue-only, the size query included: every call takes one turn at the engine's container scratch and waits for the stream
// once (decode, sizes: for the streams' chunk counts; compress: for the buffers' lengths and capacities).
#include "cj_codecs.hpp"
#include "cj_container.hpp"
#include "orc_grammar.hpp"

namespace cj {

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
// The per-chunk rows are CopyRows (cj_codecs.hpp): the codec's batch (in_base = the streams, out_base = the callers' slots) and the
// copy_segments rows of the original chunks.  cp_src != 0 marks an original chunk.

// Pass 1: the chunk count and the walk's error
__global__ __launch_bounds__(kBlockThreads) void orc_count_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                  StreamRow* st) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t nc = 0;
    const int64_t err = orc_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t, uint32_t, bool) { nc++; });
    st[i] = StreamRow{0, 0, err, err ? 0 : nc};
}

// Pass 2: the same walk writes one row per chunk; where it goes in the slot is the layout kernel's to say.  The rows were counted
// from the same bytes; should they have changed since, a chunk the count does not cover gets no row and a row the walk no longer
// reaches is an empty compressed one, which no size query accepts.
__global__ __launch_bounds__(kBlockThreads) void orc_rows_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                 const StreamRow* st, CopyRows r) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const StreamRow f = st[i];
    if (f.count == 0) return;
    uint64_t k = 0;
    const auto put = [&](uint64_t g, uint64_t at, uint32_t len, bool orig) {
        r.b.in_off[g] = at; r.b.in_len[g] = orig ? 0u : len; r.b.out_off[g] = 0; r.b.out_cap[g] = 0; r.b.result[g] = 0;
        r.cp_src[g] = orig ? (uint64_t)(uintptr_t)(in_base + at) : 0u; r.cp_dst[g] = 0; r.cp_len[g] = orig ? len : 0u;
    };
    orc_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t off, uint32_t len, bool orig) {
        if (k < f.count) { put(f.row0 + k, in_off[i] + off, len, orig); k++; }
    });
    for (; k < f.count; k++) put(f.row0 + k, in_off[i], 0u, false);
}

// One wavefront per stream, behind the codec's size query (its answers lie in the result row): the sizes of the chunks in stream
// order, 64 a round, a wave prefix sum carried across the rounds.  The first chunk in stream order whose size is an error or above
// block_size refuses the stream (the codec's code / CJ_E_ORC_BLOCK); then a total above out_cap[i] does (CJ_E_OUT_TOO_SMALL).  A
// stream that stands gets every row's place in its slot; a refused one has all its rows emptied: it decodes and copies nothing.
// out_cap == nullptr: the size query — sizes[i] = the total or the error, no row is written.
__global__ __launch_bounds__(kBlockThreads) void orc_layout_kernel(uint32_t n, StreamRow* st, CopyRows r, uint32_t block_size, const uint64_t* out_off,
                                                                   const uint64_t* out_cap, int64_t* sizes) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const uint32_t lane = lane_id();
    const StreamRow f = st[i];
    int64_t err = f.err;
    uint64_t total = 0;
    // a chunk's size: an original's length, else the query's answer
    const auto size_of = [&](uint64_t g) { return r.cp_src[g] != 0u ? (int64_t)r.cp_len[g] : r.b.result[g]; };
    for (uint64_t b = 0; err == 0 && b < f.count; b += 64u) {
        const bool in = b + lane < f.count;
        const int64_t v = in ? size_of(f.row0 + b + lane) : 0;
        const int32_t code = v < 0 ? (int32_t)v : v > (int64_t)block_size ? (int32_t)CJ_E_ORC_BLOCK : 0;
        const uint64_t bad = ballot64(in && code != 0);
        if (bad) { err = (int64_t)(int32_t)rdlane((uint32_t)code, ctz64(bad)); break; }
        total += rdlane(wave_incl_scan((uint32_t)v), 63);
    }
    if (err == 0 && out_cap != nullptr && total > out_cap[i]) err = CJ_E_OUT_TOO_SMALL;
    if (lane == 0) { st[i].err = err; st[i].total = total; }
    if (out_cap == nullptr) {
        if (lane == 0) sizes[i] = err ? err : (int64_t)total;
        return;
    }
    uint64_t pos = out_off[i];
    for (uint64_t b = 0; b < f.count; b += 64u) {
        const bool in = b + lane < f.count;
        const uint64_t g = f.row0 + b + lane;
        if (err != 0) {
            if (in) { r.b.in_len[g] = 0; r.b.out_cap[g] = 0; r.cp_len[g] = 0; }
            continue;
        }
        const bool orig = in && r.cp_src[g] != 0u;
        const uint32_t v = in ? (uint32_t)size_of(g) : 0u;
        const uint32_t inc = wave_incl_scan(v);
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
__global__ __launch_bounds__(kBlockThreads) void orc_verdict_kernel(uint32_t n, const StreamRow* st, CopyRows r, int64_t short_code, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const StreamRow f = st[i];
    int64_t res = f.err ? f.err : (int64_t)f.total;
    if (f.err == 0 && f.count) {
        const unsigned long long first = first_failing_row(f.count, [&](uint64_t k) {
            const uint64_t g = f.row0 + k;
            return r.cp_src[g] == 0u && r.b.result[g] != (int64_t)r.b.out_cap[g];
        });
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
        const uint32_t inc = wave_incl_scan(m);
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

// bytes of bound-sized chunk slots per turn of a compress batch at most: 1024 slots at the largest block size
cj::SlotBudget g_slot_budget{256ull << 20};

// out_cap == nullptr: the size query — result[i] = the sum of the chunks' sizes or the first error; nothing is decoded
int orc_decode(cj_engine* e, cj::Inner codec, uint32_t block_size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
               const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch, held across the call's one wait (cj_container.hpp)
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    cj::StreamTable t;
    int rc = cj::stream_table(turn, e, n, cj::kCopyRowWords, s, [&](cj::StreamRow* d_st) {
        hipLaunchKernelGGL(cj::orc_count_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, d_st);
    }, t);
    if (rc != 0) return rc;
    // the original chunks are copied, like the others decode, straight into the callers' slots
    cj::StreamRow* st = t.st;
    const size_t nb = t.nb;
    const cj::CopyRows r = cj::copy_rows(t.rows, nb);
    if (nb) {
        hipLaunchKernelGGL(cj::orc_rows_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, st, r);
        if ((rc = cj::inner_sizes(codec, in_base, r.b, s)) != 0) return rc;
    }
    hipLaunchKernelGGL(cj::orc_layout_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, st, r, block_size, out_off, out_cap, result);
    if (out_cap != nullptr) {
        if (nb) {
            if ((rc = cj::inner_decode(e, codec, block_size, in_base, out_base, r.b, s)) != 0) return rc;
            cj::launch_copy_segments(r.cp_src, out_base, r.cp_dst, r.cp_len, nullptr, 0, (uint32_t)nb, s);
        }
        hipLaunchKernelGGL(cj::orc_verdict_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, st, r, cj::inner_short_code(codec), result);
    }
    return turn.done(s);
}

int orc_encode(cj_engine* e, cj::Inner codec, uint32_t block_size, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
               const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // The same scratch and the same one wait, for the buffers' lengths and capacities
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    cj::EncPlan<OrcEnc> p;
    int rc = cj::enc_plan(turn, e, n, in_len, out_cap, cj::up16(cj::inner_bound(codec, block_size)), g_slot_budget, 1, s, [&](OrcEnc& x, uint64_t len, uint64_t cap, uint64_t) {
        if (len > 0x7E000000ull) x.err = CJ_E_INPUT_TOO_LARGE;
        else if (cap < cj::orc_bound(len, block_size)) x.err = CJ_E_OUT_TOO_SMALL;      // decided before any store: nothing is written
        else x.npiece = (uint32_t)((len + block_size - 1) / block_size);
    }, p);
    if (rc != 0) return rc;
    uint32_t* pick = p.extra;                   // the chunks' header words
    hipLaunchKernelGGL(cj::orc_empty_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, p.enc, result);
    rc = cj::for_turns(p, in_off, in_len, block_size, s, [](const OrcEnc*, const OrcEnc*) { return false; }, [&](uint64_t t0, uint32_t cnt, uint32_t sa, uint32_t ns) {
        const int erc = cj::inner_encode(e, codec, in_base, p.slots, p.r, cnt, s);
        if (erc != 0) return erc;
        hipLaunchKernelGGL(cj::orc_enc_layout_kernel, cj::wave_grid(ns), dim3(cj::kBlockThreads), 0, s, t0, cnt, sa, ns, p.enc, p.r.in_len, p.r.result, p.moff, pick, result);
        hipLaunchKernelGGL(cj::orc_assemble_kernel, cj::wave_grid(cnt), dim3(cj::kBlockThreads), 0, s, cnt, p.owner, pick, p.moff, in_base, p.r.in_off, p.slots, p.stride,
                           out_base, out_off);
        return 0;
    });
    if (rc != 0) return rc;
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
        return (op == CJ_OP_DECOMPRESS ? orc_decode : orc_encode)(e, cj::orc_inner(what), block_size, n_streams, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_orc_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, uint32_t block_size, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                      uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!orc_args_ok(what, op, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return (op == CJ_OP_DECOMPRESS ? orc_decode : orc_encode)(e, cj::orc_inner(what), block_size, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

int cj_orc_sizes_device(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n_streams, const uint8_t* in_base, const uint64_t* in_off,
                        const uint64_t* in_len, int64_t* result, void* hip_stream) {
    if (!size_args_ok(what, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_streams, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return orc_decode(e, cj::orc_inner(what), block_size, n_streams, in_base, in_off, in_len, nullptr, nullptr, nullptr, result, s);
    });
}

int cj_orc_sizes_host(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!size_args_ok(what, flags, block_size)) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine* e, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return orc_decode(e, cj::orc_inner(what), block_size, n, d_in, d.in_off, d.in_len, nullptr, nullptr, nullptr, d.result, s);
    });
}

// tests: the bytes of chunk slots per turn of an ORC compress batch (0 = the default); returns the previous value
uint64_t cj_debug_orc_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
