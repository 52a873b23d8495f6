// engine.hip — the C-ABI of libcramjam_hip.so (include/cramjam_hip.h): per-GPU engine, batch
// submission, host staging and the single-buffer drop-in entry points.  Host-side C++ over the HIP
// runtime; all codec arithmetic is in the four *_decode/_encode.hip kernels.  There is no CPU codec
// in this library: if no device is usable the entry points return CJ_E_NO_DEVICE.
#include "cj_stage.hpp"
#include "big_chunks.hpp"
#include "frame_grammar.hpp"

#include <atomic>

using cj::hip_ok;
using cj::parallel_chunks;

namespace {
thread_local std::string g_hip_err;
}
std::string& cj::hip_err_slot() { return g_hip_err; }

void cj::fill_args(cj::BatchArgs& a, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off,
               const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
               int64_t* result) {
    a.in_base = in_base; a.in_off = in_off; a.in_len = in_len;
    a.out_base = out_base; a.out_off = out_off; a.out_cap = out_cap;
    a.result = result; a.n_chunks = (uint32_t)n; a.flags = flags; a.hist = nullptr;
}

namespace {
std::atomic<size_t> g_grid_chunks{cj::kGridChunks};
}
size_t cj::grid_chunks() { return g_grid_chunks.load(); }
// tests: the chunks per launch of the sliced wavefront-per-chunk kernels (0 or more than kGridChunks = the default); returns the previous value
extern "C" uint64_t cj_debug_grid_chunks(uint64_t n) {
    return g_grid_chunks.exchange(n == 0 || n > cj::kGridChunks ? cj::kGridChunks : (size_t)n);
}

namespace {

#ifndef CJ_L2_WGS_PER_CU
#define CJ_L2_WGS_PER_CU 2
#endif
constexpr uint32_t kWgsPerCu = CJ_L2_WGS_PER_CU;       // persistent workgroups of the LDS decoder per CU (tuning variants change it together with CJ_L2_WINDOW)

// persistent workgroups of a batch on windows of `win` bytes: two per CU on 64 KiB windows, four / eight on the small ones
uint32_t lds_grid(const cj_engine* e, uint32_t win) { return (win >= 65536u ? kWgsPerCu : cj::lz4_lds2_wgs_per_cu(win)) * (uint32_t)e->n_cu; }

// scratch of the workgroup decoders (per-chunk verdicts, the chunk counter, record tables), shared by every call on the
// engine: a call takes a turn at it (cj::ScratchTurn) before it overwrites them
int lds_scratch(cj_engine* e, cj::ScratchTurn& turn, const cj::BatchArgs& a, hipStream_t s, bool with_sync) {
    const size_t list_bytes = 256 + cj::kClaimBytes + (size_t)a.n_chunks * 8;
    const size_t sync_bytes = with_sync ? cj::lz4_lds_scratch_sync_bytes(a.n_chunks) : 0;
    int rc;
    if ((rc = turn.reserve(e->d_sync, sync_bytes)) != 0 || (rc = turn.reserve(e->d_pmeta, cj::lz4_lds_scratch_meta_bytes(a.n_chunks))) != 0 ||
        (rc = turn.reserve(e->d_lanelist, list_bytes)) != 0) return rc;
    HIP_TRY(hipMemsetAsync(e->d_lanelist.p, 0, 256 + cj::kClaimBytes, s), CJ_E_NO_DEVICE);        // words [64 ..): the decoders' chunk counters
    if (e->n_cu == 0) HIP_TRY(hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, e->device), CJ_E_NO_DEVICE);
    // the record tables: one slot per workgroup of the largest grid that any of the three windows launches
    size_t tab_bytes = 0;
    for (const uint32_t win : {65536u, 32768u, 16384u}) tab_bytes = std::max(tab_bytes, cj::lz4_lds2_tab_bytes(lds_grid(e, win), win));
    if (!e->d_tab.reserve(tab_bytes)) return CJ_E_OOM;
    return 0;
}

// LZ4 block / Snappy raw decode of a batch of independent chunks:
//   up to CJ_FUSED_MAX_CHUNKS chunks   parse + decode in ONE kernel (two persistent workgroups per CU: segmented parse on the staged
//                      chunk, records, literals, matches through the LDS window)
//   larger batches     lane-per-chunk parse kernel (validation + sync points in memory) -> the same workgroup decoder: with every
//                      CU's LDS pipe saturated by the resolver the in-kernel parse's dependent LDS reads cost more than a second
//                      pass over the input (100 k chunks: 18 ms fused, 10.6 ms with the parse kernel)
//   then               the wavefront-per-chunk kernel on what the parse left over (errors, chunks above 64 KiB, few long runs)
//   flags              CJ_FLAG_FORCE_WAVE_PER_CHUNK / _LANE_PER_CHUNK: one mapping for every chunk (tests, comparisons)
constexpr size_t kBigCap = 8192;          // big chunks (CJ_FLAG_BIG_CHUNKS) decoded per group: each holds a record area of 1 MiB while its group is in flight
constexpr int kBigObs = 8;                // counts of big chunks the engine remembers (cj_engine::big_obs)

// CJ_FLAG_BIG_CHUNKS: which chunks lie in (64 KiB, 256 KiB] is known on the device only (big_list_kernel), but the record areas
// (1 MiB per listed chunk), the number of groups and the slab decoder's tables are decided here.  The engine sizes them from what it
// has SEEN: every flagged call copies its list's count to a pinned slot without waiting for it, and the next calls plan for the largest of
// the last kBigObs counts that have arrived.  What a batch holds beyond the plan stays with the wavefront kernel (slower, never wrong)
// and raises the plan of the calls behind it.  Only an engine that has not seen any count yet reads its first one back (the call
// waits for the stream once, like every call that grows the engine's scratch); after that a flagged call only enqueues.
int plan_big(cj_engine* e, cj_codec codec, const cj::BatchArgs& a, hipStream_t s, uint32_t** list_out, uint32_t* n_plan) {
    *n_plan = 0; *list_out = nullptr;
    const size_t big_list_bytes = ((4 + (size_t)a.n_chunks) * 4 + 255) & ~(size_t)255;
    if (!e->d_biglist.reserve(big_list_bytes)) { (void)hipGetLastError(); return 0; }      // no room for the list: the chunks stay with the wavefront kernel
    uint32_t* big_list = (uint32_t*)e->d_biglist.p;
    if (!e->h_count.p) {                                      // (h_count is set last: after a failure here the next call starts over)
        for (cj::Event& ev : e->big_ev)
            if (!ev.create()) return CJ_E_NO_DEVICE;
        if (!e->h_count.reserve(kBigObs * 4)) return CJ_E_OOM;
    }
    uint32_t* h_count = (uint32_t*)e->h_count.p;
    cj::launch_big_list(a, codec, big_list, s);
    // counts that have arrived since the last call
    bool any = false;
    uint32_t plan = 0;
    for (int i = 0; i < kBigObs; i++) {
        if (e->big_state[i] == 1 && hipEventQuery(e->big_ev[i]) == hipSuccess) { e->big_obs[i] = h_count[i]; e->big_state[i] = 2; }
        if (e->big_state[i] == 2) { any = true; plan = std::max(plan, e->big_obs[i]); }
    }
    (void)hipGetLastError();                                  // (hipErrorNotReady from the queries)
    const int slot = e->big_next;
    e->big_next = (slot + 1) % kBigObs;
    if (e->big_state[slot] == 1) HIP_TRY(hipEventSynchronize(e->big_ev[slot]), CJ_E_NO_DEVICE);   // (eight flagged calls in flight: the oldest copy must have landed before its slot is reused)
    HIP_TRY(hipMemcpyAsync(h_count + slot, big_list, 4, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipEventRecord(e->big_ev[slot], s), CJ_E_NO_DEVICE);
    e->big_state[slot] = 1;
    if (!any) {                                                // an engine that has seen nothing yet: this batch's own count
        HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
        e->big_obs[slot] = h_count[slot]; e->big_state[slot] = 2;
        plan = e->big_obs[slot];
    }
    *n_plan = (uint32_t)std::min<size_t>(plan, a.n_chunks);
    *list_out = big_list;
    return 0;
}

// d_bigmisc for a group of cap listed chunks and their kBigSlabs * cap slab work items: BigMeta x cap (256-byte aligned) | the items'
// batch rows | their ParseMeta | their done flags | the slab counter | the walk scratch.  base 0: offsets only; returns the size.
struct BigGroup { void* meta; cj::BatchRows rows; void* imeta; uint32_t* done; uint32_t* ctr; void* walk; };
size_t big_group_layout(BigGroup& g, uintptr_t base, uint32_t cap) {
    static_assert(cj::kBigItemRows == 5, "the items' descriptor rows are a BatchRows");
    const size_t items = (size_t)cj::kBigSlabs * cap;
    size_t off = 0;
    const auto region = [&](size_t bytes) { const uintptr_t p = base + off; off += bytes; return p; };
    g.meta = (void*)region((cj::big_meta_bytes(cap) + 255) & ~(size_t)255);
    g.rows = cj::batch_rows((uint64_t*)region(cj::kBigItemRows * 8 * items), items);
    g.imeta = (void*)region(8 * items);
    g.done = (uint32_t*)region(4 * items);
    g.ctr = (uint32_t*)region(256);
    g.walk = (void*)region(cj::big_walk_scratch_bytes(cap));
    return off;
}

int launch_decode(cj_engine* e, cj_codec codec, const cj::BatchArgs& a_in, hipStream_t s) {
    const bool lz4 = codec == CJ_CODEC_LZ4_BLOCK;
    cj::BatchArgs a = a_in;                                   // the batch as the kernels see it (the window promise only where it applies)
    const uint32_t small = a.flags & (CJ_FLAG_CHUNKS_LE_32K | CJ_FLAG_CHUNKS_LE_16K);
    a.flags &= ~(CJ_FLAG_CHUNKS_LE_32K | CJ_FLAG_CHUNKS_LE_16K);
    int mode = 2;
    if (a.flags & CJ_FLAG_FORCE_WAVE_PER_CHUNK) mode = 0;
    if (a.flags & CJ_FLAG_FORCE_LANE_PER_CHUNK) mode = 1;
    if (a.flags & CJ_FLAG_FORCE_LDS_PER_CHUNK) mode = 2;
    if (mode == 0) { if (lz4) cj::launch_lz4_decode(a, s); else cj::launch_snappy_decode(a, s); return 0; }
    if (mode == 1) { if (lz4) cj::launch_lz4_decode_lanes(a, s); else cj::launch_snappy_decode_lanes(a, s); return 0; }
    // the workgroup decoder (lz4_decode_lds.hip): its parse stage inside the decoder kernel for small batches, as a kernel of its own
    // in front of it for large ones (CJ_FLAG_FORCE_FUSED_PARSE / _PARSE_KERNEL: one of them at any batch size — tests, comparisons)
    bool fused = a.n_chunks <= (uint32_t)CJ_FUSED_MAX_CHUNKS;
    // (a batch of small chunks — CJ_FLAG_CHUNKS_LE_32K / _16K — runs either pipeline on windows of that size: four / eight workgroups per CU.  The
    //  one-kernel path and the parse kernel cross at ~16 k chunks for 64, 32, 16 and 8 KiB chunks alike: profiles/r06/experiments f04 / f05)
    if (a.flags & CJ_FLAG_FORCE_FUSED_PARSE) fused = true;
    if (a.flags & CJ_FLAG_FORCE_PARSE_KERNEL) fused = false;
    a.flags |= small;                                         // (round 6, f05: the one-kernel path runs on the batch's window too)
    const uint32_t win = cj::lds_window(a.flags);
    // (first: it makes `s` wait for the previous user of the engine's shared scratch — the big-chunk list below is part of it)
    cj::ScratchTurn turn(e->scratch, s);
    if (turn.rc != 0) return turn.rc;
    const int rc = lds_scratch(e, turn, a, s, !fused);
    if (rc != 0) return rc;
    uint32_t n_big = 0;
    uint32_t* big_list = nullptr;
    if (a.flags & CJ_FLAG_BIG_CHUNKS) {
        const int brc = plan_big(e, codec, a, s, &big_list, &n_big);
        if (brc != 0) return brc;
    }
    uint32_t* lists = (uint32_t*)e->d_lanelist.p;
    const uint32_t grid = lds_grid(e, win);
    if (fused) {
        cj::launch_lz4_decode_fused(a, e->d_pmeta.p, e->d_tab.p, lists + 64, grid, s, codec, win);
    } else {
        HIP_TRY(hipMemsetAsync(e->d_pmeta.p, 0, cj::lz4_lds_scratch_meta_bytes(a.n_chunks), s), CJ_E_NO_DEVICE);   // no chunk is pre-routed
        // validate, size, count sequences, sync points, route
        if (lz4) cj::launch_lz4_parse(a, e->d_sync.p, e->d_pmeta.p, s);
        else cj::launch_snappy_parse(a, e->d_sync.p, e->d_pmeta.p, s);
        cj::launch_lz4_decode_lds2(a, e->d_sync.p, e->d_pmeta.p, e->d_tab.p, lists + 64, grid, s, codec, win);
    }
    if (n_big != 0u) {
        // chunks of 64 KiB .. 256 KiB (flagged kRouteWave above): listed, parsed by 32 lanes each into records, decoded slab by slab
        // with two workgroups per CU (big_chunks.hpp) — in GROUPS of `cap` listed chunks, as many as there are record areas for
        // (1 MiB each); what that stage does not take stays flagged for the wavefront kernel
        const uint32_t cap = (uint32_t)std::min<size_t>(n_big, kBigCap);
        const uint32_t items = cj::kBigSlabs * cap;
        // the slab decoder's persistent workgroups and their tables, 0.9 MiB each (per workgroup: a slab's records + at most one extra record each
        // — the literals of a match that is cut at the slab's start — and at most one cross copy each; no forwarding in this mode: nothing stages the input)
        cj::SlabTabs tt = {std::min(cj::kBigSlabWgsPerCu * (uint32_t)e->n_cu, items), 2u * (cj::kBigSlabRecs + 64u), cj::kBigSlabRecs + 64u};
        BigGroup g;
        const size_t misc_bytes = big_group_layout(g, 0, cap);
        // no room for the record areas: the chunks stay with the wavefront kernel (slower, never wrong)
        const bool room = e->d_bigrecs.reserve_exact(cj::big_recs_bytes(cap)) && e->d_bigmisc.reserve(misc_bytes) && e->d_bigslabtab.reserve(tt.bytes());
        if (!room) (void)hipGetLastError();
        big_group_layout(g, (uintptr_t)e->d_bigmisc.p, cap);
        tt.tabs = e->d_bigslabtab.p;
        for (uint32_t base = 0; room && base < n_big; base += cap) {
            HIP_TRY(hipMemsetAsync(g.ctr, 0, 256, s), CJ_E_NO_DEVICE);
            cj::launch_big_parse(a, codec, big_list, base, cap, e->d_bigrecs.p, g.meta, e->d_pmeta.p, g.walk, s);
            cj::launch_big_items(a, big_list, base, g.meta, e->d_bigrecs.p, cap, g.rows.in_off, g.imeta, g.done, s);
            cj::BatchArgs it;
            cj::fill_args(it, a.flags & CJ_FLAG_DEBUG_PROFILE, a.in_base, a.out_base, g.rows);
            cj::launch_lz4_decode_big_slabs(it, g.imeta, e->d_bigrecs.p, g.meta, cap, g.ctr, g.done, tt, s, codec);
        }
    }
    if (lz4) cj::launch_lz4_decode_routed(a, e->d_pmeta.p, s);                // few long runs / oversize chunks / errors
    else cj::launch_snappy_decode_routed(a, e->d_pmeta.p, s);
    return turn.done(s);
}

// LZ4 block / Snappy raw encode of a batch of independent chunks: one workgroup of two wavefronts per chunk (lz4_encode.hip)
int launch_encode(cj_engine*, cj_codec codec, const cj::BatchArgs& a, hipStream_t s) {
    HIP_TRY(codec == CJ_CODEC_LZ4_BLOCK ? cj::launch_lz4_encode(a, s) : cj::launch_snappy_encode(a, s), CJ_E_NO_DEVICE);
    return 0;
}

int launch_slice(cj_engine* e, cj_codec codec, cj_op op, const cj::BatchArgs& a, hipStream_t s) {
    if (codec != CJ_CODEC_LZ4_BLOCK && codec != CJ_CODEC_SNAPPY_RAW) return CJ_E_BAD_ARG;
    const int rc = op == CJ_OP_DECOMPRESS ? launch_decode(e, codec, a, s) : launch_encode(e, codec, a, s);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

}  // namespace

// Very large batches are submitted in slices: the lane-per-chunk kernels lose efficiency when several hundred
// thousand chunks are in flight at once (their random match reads thrash L2 and the write amplification grows:
// 1 M chunks in one go ran at 299 GB/s vs 430 GB/s at 100 k), and the parse/LDS scratch stays bounded.

int cj::launch(cj_engine* e, cj_codec codec, cj_op op, const cj::BatchArgs& a, hipStream_t s) {
#ifdef CJ_DEBUG_KNOBS
    static const size_t kSliceChunks = [] {                   // (tuning builds only: the shipped library reads no environment)
        const char* v = std::getenv("CJ_SLICE_CHUNKS");
        size_t x = v ? (size_t)std::strtoull(v, nullptr, 10) : (size_t)CJ_SLICE_CHUNKS_DEFAULT;
        return x < 8192 ? (size_t)8192 : x;
    }();
#else
    constexpr size_t kSliceChunks = CJ_SLICE_CHUNKS_DEFAULT;
#endif
    if (op != CJ_OP_DECOMPRESS || a.n_chunks <= kSliceChunks) return launch_slice(e, codec, op, a, s);
    for (size_t start = 0; start < a.n_chunks; start += kSliceChunks) {
        cj::BatchArgs b = a;
        b.in_off += start; b.in_len += start; b.out_off += start; b.out_cap += start; b.result += start;
        b.n_chunks = (uint32_t)std::min(kSliceChunks, (size_t)a.n_chunks - start);
        int rc = launch_slice(e, codec, op, b, s);
        if (rc != 0) return rc;
    }
    return 0;
}

namespace {
std::once_flag g_default_once;
cj_engine* g_default = nullptr;
int g_default_rc = CJ_E_NO_DEVICE;
}  // namespace

cj_engine* cj::default_engine() {
    std::call_once(g_default_once, [] {
        int dev = 0;                                          // (the single-buffer entry points: device 0 of what HIP_VISIBLE_DEVICES shows)
#ifdef CJ_DEBUG_KNOBS
        if (const char* s = std::getenv("CJ_DEVICE")) dev = std::atoi(s);
#endif
        g_default_rc = cj_engine_create(dev, &g_default);
    });
    return g_default_rc == 0 ? g_default : nullptr;
}

namespace {

using cj::default_engine;
using cj::fill_args;
using cj::launch;

// single buffers above this size take large.hip's piece-parallel path (compress)
constexpr size_t kLargeMin = 65536;
// compress: already above two 4 KiB sub-pieces (sixteen wavefronts on a 64 KiB buffer instead of one: 1.7 -> 0.3 ms)
constexpr size_t kLargeMinCompress = 8192;

int64_t single(cj_codec codec, cj_op op, uint32_t flags, const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    cj_engine* e = default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    int64_t res = CJ_E_NO_DEVICE;
    const uint8_t* ins[1] = { in };
    uint8_t* outs[1] = { out };
    int rc = cj_batch_host(e, codec, op, flags, 1, ins, &n, outs, &cap, &res);
    return rc != 0 ? (int64_t)rc : res;
}

}  // namespace

namespace {

// The rows of a host batch in e->h_meta: inputs and outputs one after another, 16 bytes aligned, their sizes added to in_total / out_total
// (out_caps == nullptr: a size query, no output).  lz4_room 0 / 1 (LZ4 block compress, without / with the size prefix): the kernel gets a
// full LZ4_compressBound of room on the device; the caller's capacity applies when copying back (within_cap).  -1: the capacities as given.
cj::BatchRows lay_out(cj_engine* e, size_t n, const size_t* in_lens, const size_t* out_caps, int lz4_room, uint64_t& in_total, uint64_t& out_total) {
    e->h_meta.assign(5 * n, 0);
    const cj::BatchRows h = cj::batch_rows(e->h_meta.data(), n);
    for (size_t i = 0; i < n; i++) {
        h.in_off[i] = in_total;
        h.in_len[i] = in_lens[i];
        in_total += (in_lens[i] + 15u) & ~(uint64_t)15u;
        uint64_t dcap = out_caps ? out_caps[i] : 0;
        if (lz4_room >= 0) dcap = std::max<uint64_t>(dcap, cj_lz4_block_compress_bound(in_lens[i], lz4_room));
        h.out_off[i] = out_total;
        h.out_cap[i] = dcap;
        out_total += (dcap + 15u) & ~(uint64_t)15u;
    }
    return h;
}

// a result that does not fit the caller's capacity (LZ4 compress, which had a full bound on the device) is "Compression failed"
int64_t within_cap(int64_t r, size_t cap) { return r > 0 && (uint64_t)r > cap ? (int64_t)CJ_E_COMPRESS_FAILED : r; }

// the inputs of chunks [a0, b0) (`bytes` of staging) into their places in h_in
void pack(cj_engine* e, const cj::BatchRows& h, size_t a0, size_t b0, uint64_t bytes, const uint8_t* const* in_ptrs, const size_t* in_lens) {
    parallel_chunks(b0 - a0, bytes, [&](size_t a, size_t b) {
        for (size_t i = a0 + a; i < a0 + b; i++)
            if (in_lens[i]) std::memcpy(e->h_in.p + h.in_off[i], in_ptrs[i], in_lens[i]);
    });
}

// the results res of chunks [a0, b0) into result, their outputs from h_out (`bytes` of staging) to the caller
void scatter(cj_engine* e, const cj::BatchRows& h, size_t a0, size_t b0, uint64_t bytes, const int64_t* res, uint8_t* const* out_ptrs,
             const size_t* out_caps, int64_t* result) {
    parallel_chunks(b0 - a0, bytes, [&](size_t a, size_t b) {
        for (size_t i = a0 + a; i < a0 + b; i++) {
            result[i] = within_cap(res[i], out_caps[i]);
            if (result[i] > 0) std::memcpy(out_ptrs[i], e->h_out.p + h.out_off[i], (size_t)result[i]);
        }
    });
}

// The one-shot staging of a host batch whose rows h are laid out and whose device buffers are reserved (e->mu held): pack -> H2D of
// the data and the rows -> run -> D2H of the results -> wait -> D2H of the span that was produced -> scatter.  out_ptrs == nullptr
// (a size query): the two input rows travel, nothing comes back but the results.
int staged(cj_engine* e, const cj::BatchRows& h, uint64_t in_total, const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs,
           const size_t* out_caps, int64_t* result, const cj::HostRun& run) {
    const size_t n = h.n;
    hipStream_t s = e->stream;
    if (!e->h_in.reserve(in_total)) return CJ_E_OOM;
    const uint8_t* d_in = (const uint8_t*)e->d_in.p;
    uint8_t* d_out = out_ptrs ? (uint8_t*)e->d_out.p : nullptr;
    const cj::BatchRows d = cj::batch_rows((uint64_t*)e->d_meta.p, n);
    pack(e, h, 0, n, in_total, in_ptrs, in_lens);
    if (in_total) HIP_TRY(hipMemcpyAsync(e->d_in.p, e->h_in.p, in_total, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(d.in_off, h.in_off, (out_ptrs ? 4 : 2) * n * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);      // (the rows up to result / up to out_off)
    const int rc = run(d_in, d_out, d, s);
    if (rc != 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, d.result, n * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    if (!out_ptrs) return 0;
    // copy back only the span that was produced
    uint64_t span = 0;
    for (size_t i = 0; i < n; i++)
        if (result[i] > 0 && h.out_off[i] + (uint64_t)result[i] > span) span = h.out_off[i] + (uint64_t)result[i];
    if (!e->h_out.reserve(span)) return CJ_E_OOM;
    if (span) HIP_TRY(hipMemcpy(e->h_out.p, d_out, span, hipMemcpyDeviceToHost), CJ_E_NO_DEVICE);
    scatter(e, h, 0, n, span, result, out_ptrs, out_caps, result);
    return 0;
}

}  // namespace

int cj::host_batch(cj_engine* e, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs, const size_t* out_caps,
                   int64_t* result, int lz4_room, const cj::HostRun& run) {
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    uint64_t in_total = 0, out_total = 0;
    const cj::BatchRows h = lay_out(e, n, in_lens, out_ptrs ? out_caps : nullptr, lz4_room, in_total, out_total);
    if (!e->d_in.reserve(in_total + 16) || (out_ptrs && !e->d_out.reserve(out_total + 16)) || !e->d_meta.reserve(5 * n * 8)) return CJ_E_OOM;
    return staged(e, h, in_total, in_ptrs, in_lens, out_ptrs, out_caps, result, run);
}

namespace {

// A LARGE host batch, in slices: while slice k is uploaded and decoded on the engine's stream and slice k - 1 travels back
// on a second one, the host packs slice k + 1 into the pinned staging and scatters the slices that have arrived — the one-shot
// path below does these five things one after the other (pack, H2D, kernels, D2H, scatter: 18.8 GB/s of output for 16 384 x 64 KiB).
// h = the batch's rows, laid out by the caller; e->mu is held.
int batch_host_sliced(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, const cj::BatchRows& h, const uint8_t* const* in_ptrs, const size_t* in_lens,
                      uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result, uint64_t in_total, uint64_t out_total) {
    const size_t n = h.n;
    if (!e->h_in.reserve(in_total) || !e->h_out.reserve(out_total) || !e->h_res.reserve(n * 8)) return CJ_E_OOM;
    if (!e->stream_back.create()) return CJ_E_NO_DEVICE;
    size_t K = (size_t)((in_total + out_total) >> 26);               // ~64 MiB of traffic per slice
    K = K < 2 ? 2 : (K > 16 ? 16 : K);
    while (e->slice_ev.size() < 2 * K) {
        cj::Event ev;
        if (!ev.create()) return CJ_E_NO_DEVICE;
        e->slice_ev.push_back(std::move(ev));
    }
    uint8_t* d_in = (uint8_t*)e->d_in.p;
    uint8_t* d_out = (uint8_t*)e->d_out.p;
    const cj::BatchRows d = cj::batch_rows((uint64_t*)e->d_meta.p, n);
    int64_t* h_res = (int64_t*)e->h_res.p;
    HIP_TRY(hipMemcpyAsync(d.in_off, h.in_off, 4 * n * 8, hipMemcpyHostToDevice, e->stream), CJ_E_NO_DEVICE);     // (the rows up to result)
    std::vector<size_t> c(K + 1, n);                                 // slice k = chunks [c[k], c[k + 1]): equal shares of the output space (compress: of the bounds)
    c[0] = 0;
    for (size_t k = 1; k < K; k++) {
        const uint64_t want = out_total / K * k;
        size_t lo = c[k - 1], hi = n;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (h.out_off[mid] < want) lo = mid + 1; else hi = mid; }
        c[k] = lo;
    }
    const auto in_at = [&](size_t i) { return i < n ? h.in_off[i] : in_total; };
    const auto out_at = [&](size_t i) { return i < n ? h.out_off[i] : out_total; };
    const auto scatter_slice = [&](size_t k) { scatter(e, h, c[k], c[k + 1], out_at(c[k + 1]) - out_at(c[k]), h_res, out_ptrs, out_caps, result); };
    const auto bail = [&](int rc) { (void)hipStreamSynchronize(e->stream); (void)hipStreamSynchronize(e->stream_back); return rc; };
    size_t scattered = 0;
    for (size_t k = 0; k < K; k++) {
        const size_t a0 = c[k], b0 = c[k + 1];
        if (b0 > a0) {
            pack(e, h, a0, b0, in_at(b0) - in_at(a0), in_ptrs, in_lens);
            if (in_at(b0) > in_at(a0) && !hip_ok(hipMemcpyAsync(d_in + in_at(a0), e->h_in.p + in_at(a0), in_at(b0) - in_at(a0), hipMemcpyHostToDevice, e->stream), "hipMemcpyAsync")) return bail(CJ_E_NO_DEVICE);
            cj::BatchArgs a;
            fill_args(a, flags, d_in, d_out, d.sub(a0, b0 - a0));
            const int rc = cj::launch(e, codec, op, a, e->stream);
            if (rc != 0) return bail(rc);
        }
        if (!hip_ok(hipEventRecord(e->slice_ev[2 * k], e->stream), "hipEventRecord") || !hip_ok(hipStreamWaitEvent(e->stream_back, e->slice_ev[2 * k], 0), "hipStreamWaitEvent")) return bail(CJ_E_NO_DEVICE);
        if (b0 > a0) {
            if (!hip_ok(hipMemcpyAsync(h_res + a0, d.result + a0, (b0 - a0) * 8, hipMemcpyDeviceToHost, e->stream_back), "hipMemcpyAsync")) return bail(CJ_E_NO_DEVICE);
            if (out_at(b0) > out_at(a0) && !hip_ok(hipMemcpyAsync(e->h_out.p + out_at(a0), d_out + out_at(a0), out_at(b0) - out_at(a0), hipMemcpyDeviceToHost, e->stream_back), "hipMemcpyAsync")) return bail(CJ_E_NO_DEVICE);
        }
        if (!hip_ok(hipEventRecord(e->slice_ev[2 * k + 1], e->stream_back), "hipEventRecord")) return bail(CJ_E_NO_DEVICE);
        while (scattered < k && hipEventQuery(e->slice_ev[2 * scattered + 1]) == hipSuccess) scatter_slice(scattered++);
    }
    for (; scattered < K; scattered++) {
        if (!hip_ok(hipEventSynchronize(e->slice_ev[2 * scattered + 1]), "hipEventSynchronize")) return bail(CJ_E_NO_DEVICE);
        scatter_slice(scattered);
    }
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    return 0;
}

}  // namespace

extern "C" {

const char* cj_strerror(int64_t code) {
    switch (code) {
    case CJ_E_INPUT_TOO_LARGE: return "Compression input too long.";
    case CJ_E_COMPRESS_FAILED: return "Compression failed";
    case CJ_E_NO_PREFIX: return "Source buffer must at least contain size prefix.";
    case CJ_E_NEG_PREFIX: return "Parsed size prefix in buffer must not be negative.";
    case CJ_E_PREFIX_TOO_BIG: return "Given size parameter is too big";
    case CJ_E_OUT_TOO_SMALL: return "buffer isn't large enough to hold decompressed data";
    case CJ_E_CORRUPT: return "Decompression failed. Input invalid or too long?";
    case CJ_E_SNAPPY_EMPTY: return "snappy: corrupt input (empty)";
    case CJ_E_SNAPPY_HEADER: return "snappy: corrupt input (invalid header)";
    case CJ_E_SNAPPY_TOO_BIG: return "snappy: input buffer (size) is bigger than the maximum allowed";
    case CJ_E_SNAPPY_BUF_SMALL: return "snappy: output buffer is too small";
    case CJ_E_SNAPPY_CORRUPT: return "snappy: corrupt input";
    case CJ_E_FRAME_EOF: return "failed to fill whole buffer";
    case CJ_E_FRAME_WRITE: return "failed to write whole buffer";
    case CJ_E_SNAPPY_STREAM_HEADER: return "snappy: corrupt input (expected stream header but got unexpected chunk type byte)";
    case CJ_E_SNAPPY_CHUNK_TYPE: return "snappy: corrupt input (unsupported chunk type)";
    case CJ_E_SNAPPY_CHUNK_LEN: return "snappy: corrupt input (unsupported chunk length)";
    case CJ_E_SNAPPY_CHECKSUM: return "snappy: corrupt input (bad checksum)";
    case CJ_E_LZ4F_FRAME_TYPE: return "LZ4 error: ERROR_frameType_unknown";
    case CJ_E_LZ4F_HEADER: return "LZ4 error: ERROR_headerChecksum_invalid";
    case CJ_E_LZ4F_BLOCK_SIZE: return "LZ4 error: ERROR_maxBlockSize_invalid";
    case CJ_E_LZ4F_BLOCK_CHECKSUM: return "LZ4 error: ERROR_blockChecksum_invalid";
    case CJ_E_LZ4F_CONTENT_CHECKSUM: return "LZ4 error: ERROR_contentChecksum_invalid";
    case CJ_E_LZ4F_CONTENT_SIZE: return "LZ4 error: ERROR_frameSize_wrong";
    case CJ_E_LZ4F_INCOMPLETE: return "Finish runned before read end of compressed stream";
    case CJ_E_LZ4F_DECOMPRESS: return "LZ4 error: ERROR_decompressionFailed";
    case CJ_E_BLOSC_HEADER: return "blosc: corrupt chunk (invalid header, block table or stream length)";
    case CJ_E_BLOSC_UNSUPPORTED: return "blosc: unsupported chunk (only format version 2 with LZ4 streams; shuffle, bitshuffle or no filter)";
    case CJ_E_DEFLATE_CORRUPT: return "deflate: invalid data (zlib: invalid block type / stored block lengths / code lengths set / bit length repeat / literal/length code / distance code / distance too far back)";
    case CJ_E_DEFLATE_HEADER: return "deflate: invalid zlib or gzip header (zlib: incorrect header check / unknown compression method / invalid window size / unknown header flags set / header crc mismatch; preset dictionaries are not supported)";
    case CJ_E_DEFLATE_CHECKSUM: return "deflate: checksum mismatch (zlib: incorrect data check / incorrect length check)";
    case CJ_E_DEFLATE_EOF: return "deflate: the input ends inside the stream (zlib: incomplete or truncated stream)";
    case CJ_E_DEFLATE_TRAILING: return "deflate: bytes behind the end of the stream (zlib: unused data); one chunk is exactly one stream";
    case CJ_E_ZSTD_HEADER: return "zstd: invalid frame header (libzstd: prefix_unknown / frameParameter_unsupported / frameParameter_windowTooLarge; legacy frames are not supported)";
    case CJ_E_ZSTD_CORRUPT: return "zstd: corrupt block (libzstd: corruption_detected)";
    case CJ_E_ZSTD_CHECKSUM: return "zstd: content checksum mismatch (libzstd: checksum_wrong)";
    case CJ_E_ZSTD_SRC_SIZE: return "zstd: the input is truncated or has bytes behind the last frame (libzstd: srcSize_wrong)";
    case CJ_E_ZSTD_DICT: return "zstd: the frame names a dictionary (libzstd: dictionary_wrong); dictionaries are not supported";
    case CJ_E_ORC_HEADER: return "orc: truncated compression stream (fewer than 3 bytes where a chunk header must stand, or a chunk runs past the stream's end)";
    case CJ_E_ORC_BLOCK: return "orc: a chunk holds more decoded bytes than the compression block size";
    case CJ_E_PARQUET_HEADER: return "parquet: malformed page header (truncated, a bad varint or wire type, nesting too deep, a required field missing, a bad size, or a payload past the chunk's end)";
    case CJ_E_PARQUET_SIZE: return "parquet: a page decodes to fewer bytes than its header states";
    case CJ_E_PARQUET_CRC: return "parquet: page CRC-32 mismatch";
    case CJ_E_PARQUET_TABLE: return "parquet: inconsistent page table (a page type outside 0, 2, 3, a negative size, bad level lengths, sizes that do not sum to the chunk's length, or too many rows)";
    case CJ_E_NO_DEVICE: return "cramjam_hip: no usable HIP device (no CPU fallback exists)";
    case CJ_E_BAD_ARG: return "cramjam_hip: bad argument";
    case CJ_E_OOM: return "cramjam_hip: out of memory";
    default: return code >= 0 ? "ok" : "cramjam_hip: unknown error";
    }
}

const char* cj_last_hip_error(void) { return g_hip_err.c_str(); }
int cj_abi_version(void) { return CJ_ABI_VERSION; }

int cj_device_count(void) {
    int n = 0;
    if (!hip_ok(hipGetDeviceCount(&n), "hipGetDeviceCount")) return 0;
    return n;
}

size_t cj_lz4_block_compress_bound(size_t len, int prepend) {
    size_t b = len > 0x7E000000u ? 0 : len + len / 255 + 16;
    return prepend ? b + 4 : b;
}

int64_t cj_lz4_block_prefixed_len(const uint8_t* in, size_t n) {
    if (n < 4) return CJ_E_NO_PREFIX;
    return (int64_t)((uint32_t)in[0] | ((uint32_t)in[1] << 8) | ((uint32_t)in[2] << 16) | ((uint32_t)in[3] << 24));
}

size_t cj_snappy_raw_max_compress_len(size_t len) {
    if ((uint64_t)len > 0xFFFFFFFFull) return 0;
    uint64_t m = 32 + (uint64_t)len + (uint64_t)len / 6;
    return m > 0xFFFFFFFFull ? 0 : (size_t)m;
}

int64_t cj_snappy_raw_decompress_len(const uint8_t* in, size_t n) { return cj::snappy_varint_len(in, n); }

int cj_engine_create(int device, cj_engine** out) {
    if (!out) return CJ_E_BAD_ARG;
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n), CJ_E_NO_DEVICE);
    if (device < 0 || device >= n) { g_hip_err = "device index out of range"; return CJ_E_NO_DEVICE; }
    HIP_TRY(hipSetDevice(device), CJ_E_NO_DEVICE);
    cj_engine* e = new cj_engine();
    e->device = device;
    if (!e->stream.create()) { delete e; return CJ_E_NO_DEVICE; }
    *out = e;
    return 0;
}

void cj_engine_destroy(cj_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    delete e;
}

int cj_engine_device(const cj_engine* e) { return e ? e->device : -1; }

// the flag bits a C-ABI caller may set; everything else (piece splitting, tail reports, linked-frame parse: cj_common.hpp) belongs
// to large.hip / frame.hip, which call cj::launch directly — a stray bit would make a kernel read descriptors that are not there
static constexpr uint32_t kPublicFlags = CJ_FLAG_LZ4_SIZE_PREFIX | CJ_FLAG_FORCE_FUSED_PARSE | CJ_FLAG_FORCE_PARSE_KERNEL | CJ_FLAG_CHUNKS_LE_32K | CJ_FLAG_CHUNKS_LE_16K | CJ_FLAG_FORCE_WAVE_PER_CHUNK | CJ_FLAG_FORCE_LANE_PER_CHUNK | CJ_FLAG_FORCE_LDS_PER_CHUNK | CJ_FLAG_BIG_CHUNKS
                                         | CJ_FLAG_DEBUG_PROFILE;

int cj_batch_device(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                    const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                    uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                    int64_t* result, void* hip_stream) {
    if (!e || (flags & ~kPublicFlags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {}, hip_stream, [&](cj_engine*, hipStream_t s) {
        cj::BatchArgs a;
        fill_args(a, flags, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result);
        return launch(e, codec, op, a, s);
    });
}

int cj_engine_sync(cj_engine* e) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    return 0;
}

int cj_stream_sync(cj_engine* e, void* hip_stream) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(hip_stream ? (hipStream_t)hip_stream : e->stream), CJ_E_NO_DEVICE);
    return 0;
}

double cj_batch_device_timed(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                             const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                             uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                             int64_t* result, int reps) {
    if (!e || reps < 1 || n_chunks == 0 || n_chunks > 0xFFFFFFF0ull || (flags & ~kPublicFlags)) return -1.0;
    HIP_TRY(hipSetDevice(e->device), -1.0);
    cj::BatchArgs a;
    fill_args(a, flags, n_chunks, in_base, in_off, in_len, out_base, out_off, out_cap, result);
    hipEvent_t t0, t1;
    HIP_TRY(hipEventCreate(&t0), -1.0);
    HIP_TRY(hipEventCreate(&t1), -1.0);
    HIP_TRY(hipEventRecord(t0, e->stream), -1.0);
    for (int r = 0; r < reps; r++)
        if (launch(e, codec, op, a, e->stream) != 0) return -1.0;
    HIP_TRY(hipEventRecord(t1, e->stream), -1.0);
    HIP_TRY(hipEventSynchronize(t1), -1.0);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, t0, t1), -1.0);
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
    return (double)ms / reps;
}

int cj_batch_host(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n,
                  const uint8_t* const* in_ptrs, const size_t* in_lens,
                  uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!e || (n && (!in_ptrs || !in_lens || !out_ptrs || !out_caps || !result)) || (flags & ~kPublicFlags)) return CJ_E_BAD_ARG;
    if (n == 0) return 0;
    if (n > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    // decompress: chunks above 64 KiB (by input or by capacity) would each be one serial stream on one wavefront; up to
    // 256 MiB of them take the large-stream path together (large.hip) and the rest of the batch follows as usual
    if (op == CJ_OP_DECOMPRESS && n > 1 && !(flags & (CJ_FLAG_FORCE_WAVE_PER_CHUNK | CJ_FLAG_FORCE_LANE_PER_CHUNK | CJ_FLAG_FORCE_LDS_PER_CHUNK))) {
        std::vector<size_t> big, rest;
        size_t big_bytes = 0;
        for (size_t i = 0; i < n; i++) {
            const bool is_big = in_ptrs[i] && out_ptrs[i] && (in_lens[i] > kLargeMin || (codec == CJ_CODEC_SNAPPY_RAW
                                    ? cj_snappy_raw_decompress_len(in_ptrs[i], in_lens[i]) > (int64_t)kLargeMin
                                    : (out_caps[i] > kLargeMin && in_lens[i] > 4096)));
            if (is_big) { big.push_back(i); big_bytes += in_lens[i]; } else rest.push_back(i);
        }
        if (!big.empty() && big.size() <= 512 && big_bytes <= (256u << 20)) {      // (per-chunk host work: not for thousands of chunks)
            const int rc = cj::large_decompress_listed(e, codec, flags, big.size(), big.data(), in_ptrs, in_lens, out_ptrs, out_caps, result);
            if (rc != 0) return rc;
            if (rest.empty()) return 0;
            std::vector<const uint8_t*> ip(rest.size()); std::vector<size_t> il(rest.size()), oc(rest.size()); std::vector<uint8_t*> opp(rest.size());
            std::vector<int64_t> rr(rest.size());
            for (size_t k = 0; k < rest.size(); k++) { ip[k] = in_ptrs[rest[k]]; il[k] = in_lens[rest[k]]; opp[k] = out_ptrs[rest[k]]; oc[k] = out_caps[rest[k]]; }
            const int rc2 = cj_batch_host(e, codec, op, flags, rest.size(), ip.data(), il.data(), opp.data(), oc.data(), rr.data());
            if (rc2 != 0) return rc2;
            for (size_t k = 0; k < rest.size(); k++) result[rest[k]] = rr[k];
            return 0;
        }
        // many big chunks: the batch's own big-chunk path takes those of up to 256 KiB (big_chunks.hpp) — asked for only if there is one
        bool any_mid = false;
        for (size_t i : big) {
            const int64_t u = codec == CJ_CODEC_SNAPPY_RAW ? cj_snappy_raw_decompress_len(in_ptrs[i], in_lens[i]) : (int64_t)out_caps[i];
            if (u > (int64_t)kLargeMin && u <= (int64_t)(4u * 65536u)) { any_mid = true; break; }
        }
        if (any_mid) flags |= CJ_FLAG_BIG_CHUNKS;
    }
    if (op == CJ_OP_DECOMPRESS && n > 0) {                   // the capacities are on the host here: a batch of small chunks gets windows of its size
        size_t cap_max = 0;
        for (size_t i = 0; i < n; i++) cap_max = std::max(cap_max, out_caps[i]);
        flags &= ~(CJ_FLAG_CHUNKS_LE_32K | CJ_FLAG_CHUNKS_LE_16K);
        if (cap_max <= 16384) flags |= CJ_FLAG_CHUNKS_LE_16K; else if (cap_max <= 32768) flags |= CJ_FLAG_CHUNKS_LE_32K;
    }
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);

    uint64_t in_total = 0, out_total = 0;
    const int lz4_room = codec == CJ_CODEC_LZ4_BLOCK && op == CJ_OP_COMPRESS ? ((flags & CJ_FLAG_LZ4_SIZE_PREFIX) ? 1 : 0) : -1;
    const cj::BatchRows h = lay_out(e, n, in_lens, out_caps, lz4_room, in_total, out_total);
    if (!e->d_in.reserve(in_total + 16) || !e->d_out.reserve(out_total + 16) || !e->d_meta.reserve(5 * n * 8)) return CJ_E_OOM;

    // (a large batch: sliced, so that packing, the two directions of the link, the kernels and the scattering overlap)
    if (n >= 512 && in_total + out_total >= (128ull << 20))
        return batch_host_sliced(e, codec, op, flags, h, in_ptrs, in_lens, out_ptrs, out_caps, result, in_total, out_total);

    const auto run = [&](const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        cj::BatchArgs a;
        fill_args(a, flags, d_in, d_out, d);
        return launch(e, codec, op, a, s);
    };
    if (n > 1) return staged(e, h, in_total, in_ptrs, in_lens, out_ptrs, out_caps, result, run);

    // one chunk: nothing to pack or scatter, the copies go straight from and to the caller's buffers
    uint8_t* d_out = (uint8_t*)e->d_out.p;
    const cj::BatchRows d = cj::batch_rows((uint64_t*)e->d_meta.p, n);
    if (in_lens[0]) HIP_TRY(hipMemcpyAsync(e->d_in.p, in_ptrs[0], in_lens[0], hipMemcpyHostToDevice, e->stream), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(d.in_off, h.in_off, 4 * n * 8, hipMemcpyHostToDevice, e->stream), CJ_E_NO_DEVICE);     // (the rows up to result)
    const int rc = run((const uint8_t*)e->d_in.p, d_out, d, e->stream);
    if (rc != 0) return rc;
    HIP_TRY(hipMemcpyAsync(result, d.result, n * 8, hipMemcpyDeviceToHost, e->stream), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    result[0] = within_cap(result[0], out_caps[0]);
    if (result[0] > 0) HIP_TRY(hipMemcpy(out_ptrs[0], d_out, (size_t)result[0], hipMemcpyDeviceToHost), CJ_E_NO_DEVICE);
    return 0;
}

int64_t cj_lz4_block_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int level, int accel, int prepend) {
    (void)level; (void)accel;   // libcramjam always runs LZ4's DEFAULT mode (see header)
    const bool pre = prepend != 0;   // -1 (None) and 1 -> prefix
    if (n > 0x7FFFFFFFull || cj_lz4_block_compress_bound(n, 0) == 0) return CJ_E_INPUT_TOO_LARGE;
    if (pre && cap < 4) return CJ_E_COMPRESS_FAILED;
    if (n > kLargeMinCompress && in && out) return cj::large_lz4_compress(in, n, out, cap, pre);      // pieces compressed as a batch, stitched into one block
    return single(CJ_CODEC_LZ4_BLOCK, CJ_OP_COMPRESS, pre ? CJ_FLAG_LZ4_SIZE_PREFIX : 0u, in, n, out, cap);
}

int64_t cj_lz4_block_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int size_prepended) {
    // one large stream (by its input, or by the output size it announces): parsed and decoded slab-parallel (large.hip)
    uint64_t announced = cap;
    if (size_prepended && in && n >= 4) {
        uint32_t u; std::memcpy(&u, in, 4);
        if ((int32_t)u >= 0 && u <= cap) {
            announced = u;
            // an LZ4 length byte stands for at most 255 bytes: a block cannot decode to more than 255 n + 64 — a prefix that
            // announces more belongs to a stream whose decode fails; answer without staging gigabytes for it
            if (announced > 255ull * (uint64_t)n + 64ull) return CJ_E_CORRUPT;
        }
    }
    if ((n > kLargeMin || announced > kLargeMin) && in && out && !cj::large_few_elements(CJ_CODEC_LZ4_BLOCK, size_prepended ? CJ_FLAG_LZ4_SIZE_PREFIX : 0u, in, n, cap))
        return cj::large_decompress(CJ_CODEC_LZ4_BLOCK, size_prepended ? CJ_FLAG_LZ4_SIZE_PREFIX : 0u, in, n, out, cap);
    return single(CJ_CODEC_LZ4_BLOCK, CJ_OP_DECOMPRESS, size_prepended ? CJ_FLAG_LZ4_SIZE_PREFIX : 0u, in, n, out, cap);
}

int64_t cj_snappy_raw_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    if (n > kLargeMinCompress && in && out) return cj::large_snappy_compress(in, n, out, cap);
    return single(CJ_CODEC_SNAPPY_RAW, CJ_OP_COMPRESS, 0u, in, n, out, cap);
}

int64_t cj_snappy_raw_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    // a 3-byte copy element stands for at most 64 bytes: n bytes cannot decode to more than 22 n + 64 — a preamble that
    // announces more (and fits the caller's buffer) belongs to a stream whose decode fails
    if (in && n > 0) {
        const int64_t dn = cj_snappy_raw_decompress_len(in, n);
        if (dn > 0 && (uint64_t)dn <= cap && (uint64_t)dn > 22ull * (uint64_t)n + 64ull) return CJ_E_SNAPPY_CORRUPT;
    }
    if (in && out && (n > kLargeMin || (n > 0 && cj_snappy_raw_decompress_len(in, n) > (int64_t)kLargeMin)) && !cj::large_few_elements(CJ_CODEC_SNAPPY_RAW, 0u, in, n, cap))
        return cj::large_decompress(CJ_CODEC_SNAPPY_RAW, 0u, in, n, out, cap);
    return single(CJ_CODEC_SNAPPY_RAW, CJ_OP_DECOMPRESS, 0u, in, n, out, cap);
}

void* cj_device_alloc(cj_engine* e, size_t bytes) {
    if (!e) return nullptr;
    if (!hip_ok(hipSetDevice(e->device), "hipSetDevice")) return nullptr;
    void* p = nullptr;
    if (!hip_ok(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) return nullptr;
    return p;
}

void cj_device_free(cj_engine* e, void* p) {
    if (!e || !p) return;
    (void)hipSetDevice(e->device);
    (void)hipFree(p);
}

int cj_memcpy_h2d(cj_engine* e, void* d, const void* s, size_t n) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipMemcpy(d, s, n, hipMemcpyHostToDevice), CJ_E_NO_DEVICE);
    return 0;
}

int cj_memcpy_d2h(cj_engine* e, void* d, const void* s, size_t n) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipMemcpy(d, s, n, hipMemcpyDeviceToHost), CJ_E_NO_DEVICE);
    return 0;
}

int cj_memcpy_d2d(cj_engine* e, void* d, const void* s, size_t n) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipMemcpy(d, s, n, hipMemcpyDeviceToDevice), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipStreamSynchronize(nullptr), CJ_E_NO_DEVICE);      // (as cj_memset_dev)
    return 0;
}

// hipMemset of device memory returns before the bytes are set, and the engine's stream is non-blocking: it does not wait for the
// null stream.  A batch enqueued right behind the call could write its output first and have it overwritten with `v`.  So the
// helper waits, like its siblings: when it returns the bytes are set.
int cj_memset_dev(cj_engine* e, void* d, int v, size_t n) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipMemset(d, v, n), CJ_E_NO_DEVICE);
    if (n) HIP_TRY(hipStreamSynchronize(nullptr), CJ_E_NO_DEVICE);
    return 0;
}

}  // extern "C"

extern "C" uint64_t cj_debug_big_scratch_bytes(cj_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lock(e->scratch.mu);
    return (uint64_t)e->d_biglist.cap + e->d_bigrecs.cap + e->d_bigmisc.cap + e->d_bigslabtab.cap;
}

// ---- tests: what the engine's buffers HOLD between calls (tests/test_scratch_contents_gpu.py) --------------------------
// Every word a kernel or the host reads from the engine's scratch has to be written earlier in the same call; these exports put a known
// pattern into every buffer of cj::kEngineBufs that is not a state carrier, so that a reader in front of its writer shows in a result.
namespace {

// word w of a buffer filled with `pattern` (>= 2); tests/test_scratch_contents_gpu.py computes the same
__host__ __device__ inline uint32_t fill_word(uint64_t w, uint32_t pattern) {
    uint32_t h = (uint32_t)w * 0x9E3779B1u ^ (uint32_t)(w >> 32) * 0x85EBCA77u ^ pattern * 0xC2B2AE3Du;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}

__global__ __launch_bounds__(256) void fill_words_kernel(uint8_t* p, uint64_t bytes, uint32_t pattern) {
    const uint64_t words = (bytes + 3u) / 4u;
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256u) {
        const uint32_t h = fill_word(w, pattern);
        if (4u * w + 4u <= bytes) reinterpret_cast<uint32_t*>(p)[w] = h;
        else for (uint64_t b = 4u * w; b < bytes; b++) p[b] = (uint8_t)(h >> (8u * (b & 3u)));       // (a capacity that is no multiple of 4)
    }
}

void fill_host(uint8_t* p, size_t bytes, uint32_t pattern) {
    if (pattern < 2) { std::memset(p, pattern ? 0xFF : 0x00, bytes); return; }
    for (size_t w = 0; 4 * w < bytes; w++) {
        const uint32_t h = fill_word(w, pattern);
        std::memcpy(p + 4 * w, &h, std::min<size_t>(4, bytes - 4 * w));      // (little-endian hosts: byte b of a word = h >> 8 b, as on the device)
    }
}

// enqueue on s; the caller waits
int fill_device(void* p, size_t bytes, uint32_t pattern, hipStream_t s) {
    if (pattern < 2) { HIP_TRY(hipMemsetAsync(p, pattern ? 0xFF : 0x00, bytes, s), CJ_E_NO_DEVICE); return 0; }
    const uint64_t words = (bytes + 3) / 4;
    hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 16384)), dim3(256), 0, s, (uint8_t*)p, (uint64_t)bytes, pattern);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

// the buffers of one owner (its mutex held by the caller): wait for the scratch's last user, fill, and wait until the bytes are set — the
// engine's stream is non-blocking, a batch enqueued right behind the call must find them (the comment at cj_memset_dev)
int fill_owned(cj_engine* e, cj::BufOwner owner, uint32_t pattern, uint64_t* filled) {
    if (cj::Scratch* sc = cj::buf_scratch(e, owner)) {
        if (sc->free) HIP_TRY(hipEventSynchronize(sc->free), CJ_E_NO_DEVICE);
    } else {
        HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);            // (the calls under `mu` alone wait for their own work before they return)
    }
    for (int i = 0; i < cj::kEngineBufCount; i++) {
        const cj::EngineBuf& b = cj::kEngineBufs[i];
        if (b.owner != owner || b.carries_state) continue;
        if (b.dev) {
            const cj::DevBuf& d = e->*(b.dev);
            if (!d.p || !d.cap) continue;
            const int rc = fill_device(d.p, d.cap, pattern, e->stream);
            if (rc != 0) return rc;
            filled[i] = d.cap;
        } else {
            const cj::PinnedBuf& h = e->*(b.pin);
            if (!h.p || !h.cap) continue;
            fill_host(h.p, h.cap, pattern);
            filled[i] = h.cap;
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    return 0;
}

}  // namespace

extern "C" {

int cj_debug_scratch_count(void) { return cj::kEngineBufCount; }

const char* cj_debug_scratch_name(int i) { return i >= 0 && i < cj::kEngineBufCount ? cj::kEngineBufs[i].name : nullptr; }

int cj_debug_scratch_carries_state(int i) { return i >= 0 && i < cj::kEngineBufCount ? (cj::kEngineBufs[i].carries_state ? 1 : 0) : -1; }

int cj_debug_scratch_fill(cj_engine* e, uint32_t pattern, uint64_t* filled) {
    if (!filled) return CJ_E_BAD_ARG;
    if (!e) e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    for (int i = 0; i < cj::kEngineBufCount; i++) filled[i] = 0;
    // the LOCK ORDER of cj_engine.hpp: mu -> fb -> {scratch, zstd_slots, deflate_slots} one after another; dict_stage and zstd_enc_slots under mu alone
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (!e->stream.create()) return CJ_E_NO_DEVICE;
    int rc = fill_owned(e, cj::kOwnMu, pattern, filled);
    if (rc != 0) return rc;
    // (the host vector of the batch rows: lay_out and the frame paths assign() it before they read it)
    uint8_t* hm = reinterpret_cast<uint8_t*>(e->h_meta.data());
    fill_host(hm, e->h_meta.size() * 8, pattern);
    {
        std::lock_guard<std::mutex> fb(e->fb.mu);
        for (const cj::BufOwner inner : {cj::kOwnScratch, cj::kOwnZstdSlots, cj::kOwnDeflateSlots}) {
            std::lock_guard<std::mutex> in(cj::buf_scratch(e, inner)->mu);
            if ((rc = fill_owned(e, inner, pattern, filled)) != 0) return rc;
        }
        if ((rc = fill_owned(e, cj::kOwnFb, pattern, filled)) != 0) return rc;
    }
    for (const cj::BufOwner alone : {cj::kOwnDictStage, cj::kOwnZstdEncSlots}) {
        std::lock_guard<std::mutex> in(cj::buf_scratch(e, alone)->mu);
        if ((rc = fill_owned(e, alone, pattern, filled)) != 0) return rc;
    }
    return 0;
}

int cj_debug_scratch_peek(cj_engine* e, int i, uint64_t off, void* out, size_t n) {
    if (i < 0 || i >= cj::kEngineBufCount || (n && !out)) return CJ_E_BAD_ARG;
    if (!e) e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    const cj::EngineBuf& b = cj::kEngineBufs[i];
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    cj::Scratch* sc = cj::buf_scratch(e, b.owner);
    std::unique_lock<std::mutex> in;
    if (sc) {
        in = std::unique_lock<std::mutex>(sc->mu);
        if (sc->free) HIP_TRY(hipEventSynchronize(sc->free), CJ_E_NO_DEVICE);
    }
    const size_t cap = b.dev ? (e->*(b.dev)).cap : (e->*(b.pin)).cap;
    if (off > cap || n > cap - off) return CJ_E_BAD_ARG;
    if (n == 0) return 0;
    if (b.dev) HIP_TRY(hipMemcpy(out, (const uint8_t*)(e->*(b.dev)).p + off, n, hipMemcpyDeviceToHost), CJ_E_NO_DEVICE);
    else std::memcpy(out, (e->*(b.pin)).p + off, n);
    return 0;
}

}  // extern "C"
