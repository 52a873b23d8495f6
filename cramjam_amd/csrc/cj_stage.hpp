// cj_stage.hpp — the staging steps the framed (frame.hip) and large-buffer (large.hip) host paths share: the piece compressor, the
// segment assembler and the reservation of the slab decoder's tables.  The batch rows (BatchRows) are the engine's, in cj_engine.hpp;
// the slab tables' layout (SlabTabs) is the launchers', in cj_common.hpp.  The format rules stay with their callers.  Not part of the C-ABI.
#pragma once
#include "cj_engine.hpp"

#include <functional>
#include <initializer_list>

namespace cj {

void launch_crc32c_pieces(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint32_t* out, uint32_t n, hipStream_t s);
void launch_copy_segments(const uint64_t* src, uint8_t* dst_base, const uint64_t* dst_off, const uint64_t* len,
                          const uint64_t* hdr, uint32_t hdr_len, uint32_t n, hipStream_t s);      // frame_kernels.hip

// ---- batches of framed streams (frame_batch.hip host side, frame_kernels.hip device side) -------------------------------------
// One row per stream.  blk0 / slot0 come from the host's scan of the first pass; the walk's second pass fills the rest.
struct FbFrame {
    uint64_t blk0, slot0;          // first block row; offset of the stream's decoded blocks in the scratch (decompress)
    uint64_t content_size, total;  // LZ4 content size; decoded bytes the walk listed
    int64_t err, late;             // header-level error; LZ4 late error / Snappy error after the listed pieces
    uint32_t nblk, block_max;      // blocks (pieces) of the stream: pass 1's count
    uint32_t content_sum, bits;    // kFb* bits
};
constexpr uint32_t kFbIndep = 1, kFbBsum = 2, kFbCsize = 4, kFbCsum = 8, kFbSkip = 16, kFbComplete = 32;
// The per-block rows: the engine's batch (in_base = the streams, out_base = the scratch) and what the format adds
struct FbRows {
    BatchRows b;
    uint64_t *cp_src, *cp_dst, *cp_len;     // Snappy stored pieces: copy_segments rows into the scratch (len 0 elsewhere)
    uint64_t *ck_off, *ck_len;              // checksummed bytes: LZ4 block payload in the streams / Snappy piece in the scratch
    uint32_t *word, *expect, *got;          // LZ4 block word / Snappy decoded length | bit 31 stored; checksum in the stream; computed
};
constexpr size_t kFbRowWords = 13;          // u64 rows per block
inline FbRows fb_rows(uint64_t* base, size_t nb) {
    FbRows r;
    r.b = batch_rows(base, nb);
    uint64_t* p = r.b.end;
    r.cp_src = p; r.cp_dst = p + nb; r.cp_len = p + 2 * nb; r.ck_off = p + 3 * nb; r.ck_len = p + 4 * nb;
    r.word = reinterpret_cast<uint32_t*>(p + 5 * nb);
    r.expect = reinterpret_cast<uint32_t*>(p + 6 * nb);
    r.got = reinterpret_cast<uint32_t*>(p + 7 * nb);
    return r;
}
// pass 1 (cnt != nullptr: cnt[2i] = blocks, cnt[2i + 1] = scratch bytes) or pass 2 (the rows, the chain jobs of LZ4 frames with linked blocks)
void launch_fb_walk(int fmt, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint64_t* cnt,
                    FbFrame* fr, FbRows r, ChainJob* jobs, hipStream_t s);
// out[i] = XXH32(base + off[i] .. + len[i]), seed 0; one wavefront per stream
void launch_xxh32_streams(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint32_t* out, size_t n, hipStream_t s);
// decompress: the stream-order verdict of each stream, its bytes compacted into out_base + out_off[i] (LZ4: then the content checksum)
void launch_fb_finish(int fmt, size_t n, const FbFrame* fr, FbRows r, const uint8_t* in_base, const uint8_t* scratch, uint8_t* out_base,
                      const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s);
// compress: the rows of the 64 KiB pieces (fr[i].blk0 = first piece) into the scratch, `stride` bytes apart
void launch_fb_pieces(size_t n, const FbFrame* fr, const uint64_t* in_off, const uint64_t* in_len, BatchRows b, uint64_t stride, hipStream_t s);
// compress: header, block words / chunk headers, payloads (stored or from the scratch), EndMark and checksum; sums = LZ4 content XXH32
void launch_fb_assemble(int fmt, size_t n, const FbFrame* fr, FbRows r, const uint32_t* sums, const uint8_t* in_base, const uint64_t* in_len, const uint8_t* scratch, uint64_t stride, uint8_t* out_base, const uint64_t* out_off,
                        const uint64_t* out_cap, int64_t* result, hipStream_t s);

// Compress in[0, n), cut into pieces of `piece` bytes, as ONE batch into e->d_out (`stride` bytes apart), the input staged at e->d_in + H
// behind the last H bytes before it (hist: linked LZ4 blocks, kFlagLinkedEnc — piece 0 may refer to those H bytes, every other piece to
// the piece before it).  Queues the results' copy into res and, with `first`, the stitch plan kernel (first[i] = literal length of piece
// i's first sequence); the caller synchronizes.  The batch rows lie at e->d_meta (device) / e->h_meta (host); 12 rows per piece are
// reserved, the ones past batch_rows(.., np).end are the caller's.
int compress_pieces(cj_engine* e, cj_codec codec, uint32_t flags, const uint8_t* in, size_t n, size_t piece, size_t stride,
                    std::vector<int64_t>& res, std::vector<uint32_t>* first = nullptr, const uint8_t* hist = nullptr, size_t H = 0);

// One list of copy_segments rows: segment i = len bytes from the device address src to offset dst of the stream, behind the low
// hdr_len bytes of hdr
struct Segments {
    size_t n;
    uint32_t hdr_len;
    std::vector<uint64_t> rows;           // src | dst | len [| hdr], n each
    Segments(size_t n_, uint32_t hdr_len_) : n(n_), hdr_len(hdr_len_), rows((hdr_len_ ? 4 : 3) * n_, 0) {}
    void set(size_t i, const void* src, uint64_t dst, uint64_t len, uint64_t hdr = 0) {
        rows[i] = (uint64_t)(uintptr_t)src; rows[n + i] = dst; rows[2 * n + i] = len;
        if (hdr_len) rows[3 * n + i] = hdr;
    }
};

// The output of a compress path, assembled in e->d_frame and copied to out: `lead` bytes at offset 0 (the Snappy stream identifier,
// the varint of a raw stream), then every list by one upload and one copy_segments launch.  `extra` bytes behind the stream are the
// caller's: more(d_extra) queues what else writes the stream (the LZ4 stitch kernel).  Returns 0 or CJ_E_*.
template <class F>
int assemble(cj_engine* e, uint64_t size, const uint8_t* lead, size_t lead_len, std::initializer_list<const Segments*> lists,
             size_t extra, F&& more, uint8_t* out) {
    hipStream_t s = e->stream;
    const size_t tail = (size + 15u) & ~(uint64_t)15u;
    size_t rows = 0;
    for (const Segments* l : lists) rows += l->rows.size();
    if (!e->d_frame.reserve(tail + extra + rows * 8 + 64)) return CJ_E_OOM;
    uint8_t* d_frame = (uint8_t*)e->d_frame.p;
    uint64_t* d_rows = reinterpret_cast<uint64_t*>(d_frame + tail + extra);
    if (lead_len) HIP_TRY(hipMemcpyAsync(d_frame, lead, lead_len, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    for (const Segments* l : lists) {
        HIP_TRY(hipMemcpyAsync(d_rows, l->rows.data(), l->rows.size() * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
        launch_copy_segments(d_rows, d_frame, d_rows + l->n, d_rows + 2 * l->n, l->hdr_len ? d_rows + 3 * l->n : nullptr, l->hdr_len,
                             (uint32_t)l->n, s);
        d_rows += l->rows.size();
    }
    const int rc = more(d_frame + tail);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(out, d_frame, size, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    return 0;
}
inline int assemble(cj_engine* e, uint64_t size, const uint8_t* lead, size_t lead_len, std::initializer_list<const Segments*> lists, uint8_t* out) {
    return assemble(e, size, lead, lead_len, lists, 0, [](uint8_t*) { return 0; }, out);
}

// A host batch (engine.hip), the one staging of cj_batch_host, cj_frame_batch_host, cj_blosc_batch_host, cj_dict_batch_host and the size queries: under
// e->mu, on the engine's device and stream — the rows of the n buffers laid out one after another, 16 bytes aligned; the inputs packed
// into pinned staging and uploaded with the rows; run(d_in, d_out, d, s) = the device path over the device rows d; the results read
// back and waited for; the span of d_out that was produced copied back and scattered to out_ptrs (a result above its capacity becomes
// CJ_E_COMPRESS_FAILED).  out_ptrs == nullptr is a size query: no output is staged or reserved (d_out = nullptr), only in_off / in_len
// travel.  lz4_room 0 / 1: LZ4 block compress without / with the size prefix — every chunk gets at least its
// cj_lz4_block_compress_bound on the device; -1: the capacities as given.  Returns 0 or CJ_E_*.
using HostRun = std::function<int(const uint8_t* d_in, uint8_t* d_out, const BatchRows& d, hipStream_t s)>;
int host_batch(cj_engine* e, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs, const size_t* out_caps,
               int64_t* result, int lz4_room, const HostRun& run);

// ---- what the C-ABI batch entries do behind their own checks of kind, op, flags, params and dictionary -----------------------------
// The gate: the limit, every row pointer of `rows` present when n > 0, n == 0 -> 0.  kBatchGo: the call goes on.
constexpr int kBatchGo = 1;
inline int batch_gate(size_t n, std::initializer_list<const void*> rows) {
    if (n > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    for (const void* r : rows)
        if (n && !r) return CJ_E_BAD_ARG;
    return n == 0 ? 0 : kBatchGo;
}
// the scan of the entries that scan: no chunk with a length (a capacity) and no address
inline bool chunk_ptrs_ok(size_t n, const uint8_t* const* ptrs, const size_t* lens) {
    for (size_t i = 0; i < n; i++)
        if (lens[i] && !ptrs[i]) return false;
    return true;
}
// a cj_deflate_wrap that exists (the DEFLATE entries' own check, decode and compress)
inline bool deflate_wrap_ok(int wrap) { return wrap == CJ_DEFLATE_RAW || wrap == CJ_DEFLATE_ZLIB || wrap == CJ_DEFLATE_GZIP; }
// A device call: the gate, the engine (nullptr: the default one) and its device; launch(e, s) enqueues on the caller's stream or the engine's
template <class F>
int device_call(cj_engine* e, size_t n, std::initializer_list<const void*> rows, void* hip_stream, F&& launch) {
    const int g = batch_gate(n, rows);
    if (g != kBatchGo) return g;
    if (!e && !(e = default_engine())) return CJ_E_NO_DEVICE;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    return launch(e, hip_stream ? (hipStream_t)hip_stream : e->stream);
}
// A host call: the gate (scan: then the per-chunk pointers), the engine, host_batch around launch(e, d_in, d_out, d, s)
template <class F>
int host_call(cj_engine* e, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs, const size_t* out_caps,
              int64_t* result, int lz4_room, bool scan, F&& launch) {
    const int g = batch_gate(n, {in_ptrs, in_lens, out_ptrs, out_caps, result});
    if (g != kBatchGo) return g;
    if (scan && !(chunk_ptrs_ok(n, in_ptrs, in_lens) && chunk_ptrs_ok(n, out_ptrs, out_caps))) return CJ_E_BAD_ARG;
    if (!e && !(e = default_engine())) return CJ_E_NO_DEVICE;
    return host_batch(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, lz4_room,
                      [&](const uint8_t* d_in, uint8_t* d_out, const BatchRows& d, hipStream_t s) { return launch(e, d_in, d_out, d, s); });
}
// A host size query: the gate, the scan, the engine, host_batch without an output around launch(e, d_in, d, s)
template <class F>
int host_sizes_call(cj_engine* e, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result, F&& launch) {
    const int g = batch_gate(n, {in_ptrs, in_lens, result});
    if (g != kBatchGo) return g;
    if (!chunk_ptrs_ok(n, in_ptrs, in_lens)) return CJ_E_BAD_ARG;
    if (!e && !(e = default_engine())) return CJ_E_NO_DEVICE;
    return host_batch(e, n, in_ptrs, in_lens, nullptr, nullptr, result, -1,
                      [&](const uint8_t* d_in, uint8_t*, const BatchRows& d, hipStream_t s) { return launch(e, d_in, d, s); });
}

// The slab decoder's per-workgroup tables (launch_lz4_decode_lds2_slabs) for n_slabs slabs of at most max_rec records, in e->d_bigtab
int reserve_slab_tabs(cj_engine* e, size_t n_slabs, uint32_t max_rec, SlabTabs& t);

}  // namespace cj
