// frame.hip — framed container formats on top of the batch engine.
//
// Snappy framing format: what the reference reaches at /root/reference/src/snappy.rs:24 (decompress), :38
// (compress), :82 (compress_into), :88 (decompress_into) through libcramjam::snappy::{compress,decompress} ->
// snap 1.1.1 read::FrameEncoder / read::FrameDecoder.  A framed stream is a sequence of independent <= 64 KiB
// pieces, which is exactly the batch the block engine wants: the host walks the 4-byte chunk headers (a serial
// but trivial scan), the GPU decodes/encodes every piece in one batch, checksums every piece (crc32c_pieces) and
// assembles the stream (copy_segments).  No codec or checksum arithmetic runs on the host.
#include "cj_stage.hpp"
#include "xxh32_host.hpp"
#include "lz4_lane_walk.hpp"
#include "frame_grammar.hpp"

#include <atomic>

namespace {
// (tuning builds only: every linked-block frame through the chain kernel; the shipped library reads no environment)
inline bool lz4f_chain_only() {
#ifdef CJ_DEBUG_KNOBS
    static const bool v = std::getenv("CJ_LZ4F_CHAIN_ONLY") != nullptr;
    return v;
#else
    return false;
#endif
}

constexpr size_t kPiece = cj::kSnapPiece;
constexpr size_t kTmpStride = 76496;      // cj::kSnapMaxChunk rounded up to 16
const uint8_t kIdent[10] = { 0xff, 0x06, 0x00, 0x00, 's', 'N', 'a', 'P', 'p', 'Y' };

using Piece = cj::SnapPiece;

}  // namespace

extern "C" {

size_t cj_snappy_frame_max_compress_len(size_t n) {
    if (n == 0) return 0;
    return 10 + ((n + kPiece - 1) / kPiece) * 8 + n;
}

int64_t cj_snappy_frame_decompress_len(const uint8_t* in, size_t n) {
    if (n && !in) return CJ_E_BAD_ARG;
    return cj::snappy_frame_len(in, n);
}

int64_t cj_snappy_frame_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    if ((n && !in) || (cap && !out)) return CJ_E_BAD_ARG;
    cj_engine* e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    std::vector<Piece> pieces;
    uint64_t total = 0;
    const int64_t gerr = cj::snappy_frame_walk(in, n, [&](const Piece& p) { pieces.push_back(p); }, &total);
    const size_t np = pieces.size();
    if (np == 0) return gerr;
    if (np > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    size_t nc = 0;
    for (const Piece& p : pieces) nc += p.stored ? 0 : 1;
    const size_t ns = np - nc;

    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    // device meta rows (u64): compressed pieces in_off|in_len|out_off|out_cap|result (nc each), stored pieces
    // src|dst_off|len (ns each), all pieces off|len (np each), then np u32 checksums
    const size_t r_s = 5 * nc, r_p = r_s + 3 * ns, r_crc = r_p + 2 * np, rows = r_crc + (np + 1) / 2;
    if (!e->d_frame.reserve(n + 16) || !e->d_out.reserve(total + 16) || !e->d_meta.reserve(rows * 8)) return CJ_E_OOM;
    uint8_t* d_in = (uint8_t*)e->d_frame.p;
    uint8_t* d_out = (uint8_t*)e->d_out.p;
    uint64_t* d_meta = (uint64_t*)e->d_meta.p;
    std::vector<uint64_t>& m = e->h_meta;
    m.assign(rows, 0);
    const cj::BatchRows mc = cj::batch_rows(m.data(), nc), dc = cj::batch_rows(d_meta, nc);
    size_t ci = 0, si = 0;
    for (size_t i = 0; i < np; i++) {
        const Piece& p = pieces[i];
        if (p.stored) {
            m[r_s + si] = (uint64_t)(uintptr_t)(d_in + p.src_off);
            m[r_s + ns + si] = p.dst_off;
            m[r_s + 2 * ns + si] = p.dst_len;
            si++;
        } else {
            mc.in_off[ci] = p.src_off;
            mc.in_len[ci] = p.src_len;
            mc.out_off[ci] = p.dst_off;
            mc.out_cap[ci] = p.dst_len;             // snap decodes into dst[..decompress_len]
            ci++;
        }
        m[r_p + i] = p.dst_off;
        m[r_p + np + i] = p.dst_len;
    }
    hipStream_t s = e->stream;
    HIP_TRY(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(d_meta, m.data(), r_crc * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    if (nc) {
        cj::BatchArgs a;
        cj::fill_args(a, 0, d_in, d_out, dc);
        const int rc = cj::launch(e, CJ_CODEC_SNAPPY_RAW, CJ_OP_DECOMPRESS, a, s);
        if (rc != 0) return rc;
    }
    cj::launch_copy_segments(d_meta + r_s, d_out, d_meta + r_s + ns, d_meta + r_s + 2 * ns, nullptr, 0, (uint32_t)ns, s);
    cj::launch_crc32c_pieces(d_out, d_meta + r_p, d_meta + r_p + np, (uint32_t*)(d_meta + r_crc), (uint32_t)np, s);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    std::vector<int64_t> res(nc);
    std::vector<uint32_t> crc(np);
    if (nc) HIP_TRY(hipMemcpyAsync(res.data(), dc.result, nc * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(crc.data(), d_meta + r_crc, np * 4, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);

    // first failure in stream order: block error, checksum, then the writer running out of room
    ci = 0;
    uint64_t written = 0;
    for (size_t i = 0; i < np; i++) {
        const Piece& p = pieces[i];
        if (!p.stored) {
            const int64_t r = res[ci++];
            if (r < 0) return r;
        }
        if (crc[i] != p.crc) return CJ_E_SNAPPY_CHECKSUM;
        if (out != nullptr && written + p.dst_len > cap) return CJ_E_FRAME_WRITE;
        written += p.dst_len;
    }
    if (gerr) return gerr;
    if (out != nullptr && total) HIP_TRY(hipMemcpy(out, d_out, total, hipMemcpyDeviceToHost), CJ_E_NO_DEVICE);
    return (int64_t)total;
}

int64_t cj_snappy_frame_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    if ((n && !in) || (cap && !out)) return CJ_E_BAD_ARG;
    cj_engine* e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    if (n == 0) return 0;                  // snap emits the stream identifier together with the first chunk only
    const size_t np = (n + kPiece - 1) / kPiece;
    if (np > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    if (n > 8192 && n <= cj::large_split_max()) return cj::large_snappy_frame(in, n, out, cap);     // sub-pieces, one wavefront each (large.hip)

    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    hipStream_t s = e->stream;
    std::vector<int64_t> res;
    int rc = cj::compress_pieces(e, CJ_CODEC_SNAPPY_RAW, 0u, in, n, kPiece, kTmpStride, res);
    if (rc != 0) return rc;
    const uint8_t* d_in = (const uint8_t*)e->d_in.p;
    const uint8_t* d_tmp = (const uint8_t*)e->d_out.p;
    const cj::BatchRows d = cj::batch_rows((uint64_t*)e->d_meta.p, np);
    uint32_t* d_crc = reinterpret_cast<uint32_t*>(d.end);
    cj::launch_crc32c_pieces(d_in, d.in_off, d.in_len, d_crc, (uint32_t)np, s);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    std::vector<uint32_t> crc(np);
    HIP_TRY(hipMemcpyAsync(crc.data(), d_crc, np * 4, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);

    // chunk layout (snap frame.rs compress_frame): stored when compressed_len >= len - len/8
    cj::Segments seg(np, 8);
    uint64_t fpos = 10;
    for (size_t i = 0; i < np; i++) {
        if (res[i] < 0) return res[i];
        const uint64_t len = std::min(kPiece, n - i * kPiece), cl = (uint64_t)res[i];
        const bool stored = cl >= len - len / 8;
        const uint64_t body = stored ? len : cl;
        seg.set(i, stored ? d_in + i * kPiece : d_tmp + i * kTmpStride, fpos + 8, body, (stored ? 1ull : 0ull) | ((body + 4) << 8) | ((uint64_t)crc[i] << 32));
        fpos += 8 + body;
    }
    if (fpos > cap) return CJ_E_FRAME_WRITE;
    rc = cj::assemble(e, fpos, kIdent, 10, {&seg}, out);
    return rc != 0 ? rc : (int64_t)fpos;
}

// =====================================================================================================================
// LZ4 FRAME format: what the reference reaches at /root/reference/src/lz4.rs:28 (decompress), :43 (compress), :56
// (compress_into), :63 (decompress_into) through libcramjam::lz4::{compress,decompress} -> lz4 crate Encoder/Decoder ->
// LZ4F_* (liblz4 1.10.0).  Blocks are de/compressed on the GPU: frames with independent blocks (and single-block
// frames) as ONE batch through the block engine, frames with linked blocks by the chain kernel (lz4_decode.hip).
// The frame's XXH32 checksums are the one piece of arithmetic done on the host: XXH32 is a serial recurrence of four
// 32-bit multiply-rotate accumulators per frame — one CPU core sustains ~6 GB/s on it, one GPU wavefront ~1 GB/s
// (quarter-rate 32-bit multiplies on a dependent chain) — so it runs on a host thread concurrently with the device batch.
// =====================================================================================================================
namespace {

using cj::xxh32;
inline uint32_t xrd32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline void xwr32(uint8_t* p, uint32_t v) { std::memcpy(p, &v, 4); }

constexpr size_t kLz4fBlock = 65536;                      // the reference encoder's block size (lz4 crate BlockSize::Default)
constexpr size_t kLz4fTmpStride = 65824;                  // LZ4_compressBound(65536) = 65809, rounded up to 16

struct Lz4Block { uint64_t src_off; uint32_t word; };     // word = size | bit 31 (stored)
struct Lz4Frame : cj::Lz4Header {
    std::vector<Lz4Block> blocks;
};

// the shared walk (frame_grammar.hpp), the blocks listed; with verify_block_sums the walk stops at the first bad block checksum
int64_t lz4_frame_walk(const uint8_t* in, size_t n, Lz4Frame& f, bool verify_block_sums) {
    return cj::lz4_frame_walk(in, n, f, [&](uint64_t pos, uint32_t w) {
        const size_t sz = w & 0x7FFFFFFFu;
        if (f.bsum && verify_block_sums && xrd32(in + pos + sz) != xxh32(in + pos, sz, 0)) return false;
        f.blocks.push_back({pos, w});
        return true;
    });
}

}  // namespace

namespace {

std::atomic<unsigned long long> g_linked_lds_frames{0};

// Linked 64 KiB blocks through parse + lz4_decode_lds2_kernel<LZ4, linked>: ~100x the chain kernel on short-sequence data.
// Needs every non-last block to decode to exactly 64 KiB (block k then starts at k * 64 KiB and its history is the whole
// previous block) and every block to fit the LDS decoder (<= 16 384 sequences, <= 65 504 input bytes); the parse kernel
// establishes both.  Returns 0 when the frame was decoded this way, 1 when the caller must fall back to the chain
// kernel, < 0 on a device error.
int lz4_frame_linked_lds(cj_engine* e, const Lz4Frame& f, const uint8_t* d_in, std::vector<int64_t>& res, uint8_t** d_final) {
    const size_t nb = f.blocks.size();
    const uint64_t B = 65536;
    hipStream_t s = e->stream;
    cj::ScratchTurn turn(e->scratch, s);       // (no done(): the call waits for its own kernels, the next turn has nobody to wait for)
    if (turn.rc != 0 || (turn.rc = turn.wait_host()) != 0) return turn.rc;
    // rows: in_off | in_len | out_off | out_cap | result | hist(u32) | frames(uint2) | first(uint2 per block) | counter | done(u32 per block)
    const size_t hw = (nb * 4 + 7) / 8, r_first = 5 * nb + hw + 1, r_cnt = r_first + nb, r_done = r_cnt + 1, rows = r_done + hw;
    const size_t list_bytes = 16;
    if (!e->d_out.reserve(nb * B + 16) || !e->d_meta.reserve(rows * 8) || !e->d_sync.reserve(cj::lz4_lds_scratch_sync_bytes(nb)) ||
        !e->d_pmeta.reserve(cj::lz4_lds_scratch_meta_bytes(nb)) || !e->d_lanelist.reserve(list_bytes) ||
        !e->d_tab.reserve(cj::lz4_lds2_tab_bytes(1))) return CJ_E_OOM;
    uint64_t* d_meta = (uint64_t*)e->d_meta.p;
    std::vector<uint64_t>& m = e->h_meta;
    m.assign(rows, 0);
    const cj::BatchRows mb = cj::batch_rows(m.data(), nb), d = cj::batch_rows(d_meta, nb);
    uint32_t* hist = reinterpret_cast<uint32_t*>(mb.end);
    for (size_t i = 0; i < nb; i++) {
        const Lz4Block& b = f.blocks[i];
        mb.in_off[i] = b.src_off;
        mb.in_len[i] = (uint64_t)(b.word & 0x7FFFFFFFu) | ((b.word & 0x80000000u) ? (1ull << 63) : 0ull);
        mb.out_off[i] = i * B;
        mb.out_cap[i] = B;
        hist[i] = i ? 65536u : 0u;
    }
    uint32_t* fr = reinterpret_cast<uint32_t*>(mb.end + hw);
    fr[0] = 0u; fr[1] = (uint32_t)nb;
    uint32_t* first = reinterpret_cast<uint32_t*>(m.data() + r_first);
    for (size_t i = 0; i < nb; i++) { first[2 * i] = (uint32_t)(i * cj::kSyncPitch); first[2 * i + 1] = 0u; }
    HIP_TRY(hipMemcpyAsync(d_meta, m.data(), rows * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemsetAsync(e->d_pmeta.p, 0, cj::lz4_lds_scratch_meta_bytes(nb), s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemsetAsync(e->d_lanelist.p, 0, 16, s), CJ_E_NO_DEVICE);
    cj::BatchArgs a;
    cj::fill_args(a, cj::kFlagLinkedFrame, d_in, (uint8_t*)e->d_out.p, d);
    a.hist = reinterpret_cast<const uint32_t*>(d.end);
    cj::launch_lz4_parse(a, e->d_sync.p, e->d_pmeta.p, s);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    std::vector<uint64_t> pmeta(nb);
    HIP_TRY(hipMemcpyAsync(res.data(), d.result, nb * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(pmeta.data(), e->d_pmeta.p, nb * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    for (size_t i = 0; i < nb; i++) {
        const uint32_t in_skip = (uint32_t)(pmeta[i] >> 32);          // ParseMeta {nseq, in_skip}
        if (res[i] < 0 || (in_skip & 0x80000000u)) return 1;          // malformed (the chain kernel names the block) or not LDS-capable
        if (i + 1 < nb && (uint64_t)res[i] != B) return 1;            // a short block in the middle: positions are not k * 64 KiB
        if (res[i] == 0 && !(in_skip & 0x20000000u)) return 1;
    }
#ifdef CJ_DEBUG_KNOBS
    static const bool one_wg = std::getenv("CJ_LZ4F_ONE_WORKGROUP") != nullptr;      // (tuning builds only: the older one-workgroup path, tests/perf/linked_frame_rate.py)
#else
    constexpr bool one_wg = false;
#endif
    if (one_wg) {
        // one workgroup walks the frame's blocks in order, the previous block in a second LDS window
        cj::launch_lz4_decode_lds2_linked(a, e->d_sync.p, e->d_pmeta.p, e->d_tab.p, (uint32_t*)e->d_lanelist.p + 2,
                                          d.end + hw, 1u, 1u, s);
    } else {
        // every block is a slab of the large-stream decoder (large.hip / DESIGN 5.6): two workgroups per CU take the blocks in
        // order, a match that reaches into earlier blocks is copied from their finished output once the predecessor's
        // completion flag is up, everything else is resolved meanwhile
        cj::SlabTabs tt;
        const int rc = cj::reserve_slab_tabs(e, nb, cj::kSyncStride * cj::kSyncEvery, tt);
        if (rc != 0) return rc;
        cj::launch_lz4_decode_lds2_slabs(a, e->d_sync.p, e->d_pmeta.p, (uint32_t*)(d_meta + r_cnt), d_meta + r_first, 0u,
                                         (uint32_t*)(d_meta + r_done), tt, s, CJ_CODEC_LZ4_BLOCK, true);
    }
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(res.data(), d.result, nb * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);     // the decoder's stall guard reports here
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    *d_final = (uint8_t*)e->d_out.p;
    g_linked_lds_frames.fetch_add(1);
    return 0;
}

}  // namespace

// debug aid (tests): number of linked-block frames decoded by the two-window LDS decoder in this process
extern "C" unsigned long long cj_debug_linked_lds_frames(void) { return g_linked_lds_frames.load(); }

size_t cj_lz4_frame_compress_bound(size_t n) {
    return 7 + ((n + kLz4fBlock - 1) / kLz4fBlock) * 4 + n + 4 + 4;
}

int64_t cj_lz4_frame_decompress_bound(const uint8_t* in, size_t n) {
    if (n && !in) return CJ_E_BAD_ARG;
    return cj::lz4_frame_bound(in, n);          // (one rule for the host and for the device query: frame_grammar.hpp)
}

namespace {
// The block sequence of a frame (u32 size word + data per 64 KiB of input, no header, no EndMark) written to out.  Linked blocks: block
// k may refer to the 64 KiB of input before it — the last <= 64 KiB of hist for block 0 — staged as hist | in on the device, so every
// block still is one independent chunk of the batch (kFlagLinkedEnc: its history is indexed before its walk).  Linked blocks always take
// the batch kernel: the split pieces (large.hip) restart their walk every 4 KiB, and a sub-piece whose matches lie ~64 KiB back rarely
// finds them — their hash slots have gone to the 64 K positions after them — where one walk through the block needs a single hit (64 KiB
// of random bytes twice: 0.502 of the independent frame in one walk, ~0.57 in sub-pieces).
int64_t lz4_frame_blocks(const uint8_t* hist, size_t hist_len, const uint8_t* in, size_t n, uint8_t* out, size_t cap, bool linked) {
    if ((n && !in) || (cap && !out) || (hist_len && !hist)) return CJ_E_BAD_ARG;
    cj_engine* e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    const size_t np = (n + kLz4fBlock - 1) / kLz4fBlock;
    if (np > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    if (np == 0) return 0;
    const size_t H = linked ? std::min(hist_len, kLz4fBlock) : 0;        // only the last 64 KiB before the block can be referred to
    if (H) hist += hist_len - H;
    // up to 32 MiB: sixteen (above 16 MiB: four) wavefronts per 64 KiB block (sub-pieces joined into one LZ4 block, large.hip) —
    // one wavefront per block would make every call at least the 1.7 ms it needs for 64 KiB
    if (!linked && n > 8192 && n <= cj::large_split_max()) return cj::large_lz4_frame_blocks(in, n, out, cap);
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    std::vector<int64_t> res;
    int rc = cj::compress_pieces(e, CJ_CODEC_LZ4_BLOCK, linked ? cj::kFlagLinkedEnc : 0u, in, n, kLz4fBlock, kLz4fTmpStride, res, nullptr, hist, H);
    if (rc != 0) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    const uint8_t* d_blk = (const uint8_t*)e->d_in.p + H;            // block i starts at d_blk + i * 64 KiB
    const uint8_t* d_tmp = (const uint8_t*)e->d_out.p;
    // LZ4F_makeBlock: a block that does not shrink is stored (bit 31 of the size word)
    cj::Segments seg(np, 4);
    uint64_t fpos = 0;
    for (size_t i = 0; i < np; i++) {
        if (res[i] < 0) return res[i];
        const uint64_t len = std::min(kLz4fBlock, n - i * kLz4fBlock), cl = (uint64_t)res[i];
        const bool stored = cl >= len;
        const uint64_t body = stored ? len : cl;
        seg.set(i, stored ? d_blk + i * kLz4fBlock : d_tmp + i * kLz4fTmpStride, fpos + 4, body, body | (stored ? 0x80000000ull : 0ull));
        fpos += 4 + body;
    }
    if (fpos > cap) return CJ_E_FRAME_WRITE;
    rc = cj::assemble(e, fpos, nullptr, 0, {&seg}, out);
    return rc != 0 ? rc : (int64_t)fpos;
}

// header + blocks + EndMark + content checksum; FLG 0x64 (independent blocks) or 0x44 (linked), BD 0x40 (64 KiB blocks)
int64_t lz4_frame(const uint8_t* in, size_t n, uint8_t* out, size_t cap, bool linked) {
    if ((n && !in) || (cap && !out)) return CJ_E_BAD_ARG;
    if (!cj::default_engine()) return CJ_E_NO_DEVICE;
    if (cap < 15) return CJ_E_FRAME_WRITE;
    uint8_t hdr[7] = { 0x04, 0x22, 0x4D, 0x18, (uint8_t)(linked ? 0x44 : 0x64), 0x40, 0 };
    hdr[6] = (uint8_t)(xxh32(hdr + 4, 2, 0) >> 8);
    std::memcpy(out, hdr, 7);
    uint32_t content_sum = 0;
    std::thread summer([&] { content_sum = xxh32(in, n, 0); });          // overlaps the device batch
    const int64_t r = lz4_frame_blocks(nullptr, 0, in, n, out + 7, cap - 15, linked);
    summer.join();
    if (r < 0) return r;
    xwr32(out + 7 + r, 0u);                  // EndMark
    xwr32(out + 11 + r, content_sum);
    return r + 15;
}
}  // namespace

int64_t cj_lz4_frame_compress_blocks(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    return lz4_frame_blocks(nullptr, 0, in, n, out, cap, false);
}

int64_t cj_lz4_frame_compress_blocks_linked(const uint8_t* hist, size_t hist_len, const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    return lz4_frame_blocks(hist, hist_len, in, n, out, cap, true);
}

int64_t cj_lz4_frame_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int level) {
    (void)level;                           // the GPU matcher has one mode; any level yields a valid frame (see header)
    return lz4_frame(in, n, out, cap, false);
}

int64_t cj_lz4_frame_compress_linked(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int level) {
    (void)level;
    return lz4_frame(in, n, out, cap, true);
}

int64_t cj_lz4_frame_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    if ((n && !in) || (cap && !out)) return CJ_E_BAD_ARG;
    cj_engine* e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    Lz4Frame f;
    const int64_t werr = lz4_frame_walk(in, n, f, true);
    if (werr) return werr;
    if (f.skippable) return 0;
    const size_t nb = f.blocks.size();
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    uint64_t total = 0;
    // Independent blocks above 64 KiB (the lz4 command line's 4 MiB default, 256 KiB / 1 MiB frames): as chunks of a batch each
    // would be one serial stream on one wavefront (0.035 GB/s per block); instead all blocks go through the large-stream
    // path together (large.hip: one parallel parse over the pieces of all blocks, one slab decoder launch over all slabs).
    bool big_done = false;
    const bool few_big = f.block_max > 65536;
    if (nb > 0 && few_big && out != nullptr && f.indep) {
        uint64_t bound = 0;
        for (const Lz4Block& b : f.blocks) bound += (b.word & 0x80000000u) ? (b.word & 0x7FFFFFFFu) : f.block_max;
        if (bound <= cap) {                                                    // (else: the generic path knows the writer's error order)
            // every compressed block decodes to its slot (where it would lie if every block before it decoded to block_max
            // bytes); the parse runs over all blocks at once; then the output is closed up where a block came out shorter
            // (only the last one does in frames liblz4 writes) and the stored blocks are copied in
            std::vector<const uint8_t*> ins; std::vector<size_t> lens, caps; std::vector<uint8_t*> outs;
            std::vector<uint64_t> slots(nb);
            uint64_t slot = 0;
            for (size_t i = 0; i < nb; i++) {
                const Lz4Block& b = f.blocks[i];
                const uint32_t sz = b.word & 0x7FFFFFFFu;
                slots[i] = slot;
                if (b.word & 0x80000000u) slot += sz;
                else { ins.push_back(in + b.src_off); lens.push_back(sz); outs.push_back(out + slot); caps.push_back(f.block_max); slot += f.block_max; }
            }
            std::vector<int64_t> rj(ins.size());
            const int rc = ins.empty() ? 0 : cj::large_decompress_many(e, CJ_CODEC_LZ4_BLOCK, ins.size(), ins.data(), lens.data(), nullptr, outs.data(), caps.data(), rj.data());
            if (rc == 0) {
                size_t k = 0;
                for (size_t i = 0; i < nb; i++) {
                    const Lz4Block& b = f.blocks[i];
                    uint64_t got;
                    if (b.word & 0x80000000u) { got = b.word & 0x7FFFFFFFu; std::memmove(out + total, in + b.src_off, got); }
                    else {
                        if (rj[k] < 0) return CJ_E_LZ4F_DECOMPRESS;
                        got = (uint64_t)rj[k++];
                        if (slots[i] != total) std::memmove(out + total, out + slots[i], got);
                    }
                    total += got;
                }
                big_done = true;
            } else if (rc != CJ_E_BAD_ARG) return rc;
        }
    }
    if (nb > 0 && !big_done) {
        const uint64_t B = f.block_max;
        std::lock_guard<std::mutex> lock(e->mu);
        HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
        hipStream_t s = e->stream;
        if (!e->d_frame.reserve(n + 16)) return CJ_E_OOM;
        uint8_t* d_in = (uint8_t*)e->d_frame.p;
        HIP_TRY(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
        std::vector<int64_t> res(nb);
        uint8_t* d_final = nullptr;
        if (f.indep || nb == 1) {
            // one batch: compressed blocks decode into slots of the maximal block size, then everything is compacted
            size_t nc = 0;
            for (const Lz4Block& b : f.blocks) nc += (b.word & 0x80000000u) ? 0 : 1;
            // rows: in_off|in_len|out_off|out_cap|result (nc each) | src|dst_off|len (nb each)
            const size_t r_g = 5 * nc, rows = r_g + 3 * nb;
            if (!e->d_in.reserve(nc * B + 16) || !e->d_meta.reserve(rows * 8)) return CJ_E_OOM;
            uint8_t* d_tmp = (uint8_t*)e->d_in.p;
            uint64_t* d_meta = (uint64_t*)e->d_meta.p;
            std::vector<uint64_t>& m = e->h_meta;
            m.assign(rows, 0);
            const cj::BatchRows mc = cj::batch_rows(m.data(), nc), dc = cj::batch_rows(d_meta, nc);
            size_t ci = 0;
            for (const Lz4Block& b : f.blocks) {
                if (b.word & 0x80000000u) continue;
                mc.in_off[ci] = b.src_off; mc.in_len[ci] = b.word; mc.out_off[ci] = ci * B; mc.out_cap[ci] = B;
                ci++;
            }
            std::vector<int64_t> cres(nc);
            if (nc) {
                HIP_TRY(hipMemcpyAsync(d_meta, m.data(), 4 * nc * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
                cj::BatchArgs a;
                cj::fill_args(a, 0, d_in, d_tmp, dc);
                const int rc = cj::launch(e, CJ_CODEC_LZ4_BLOCK, CJ_OP_DECOMPRESS, a, s);
                if (rc != 0) return rc;
                HIP_TRY(hipMemcpyAsync(cres.data(), dc.result, nc * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
            }
            HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
            ci = 0;
            uint64_t pos = 0;
            for (size_t i = 0; i < nb; i++) {
                const Lz4Block& b = f.blocks[i];
                const bool stored = (b.word & 0x80000000u) != 0;
                const int64_t r = stored ? (int64_t)(b.word & 0x7FFFFFFFu) : cres[ci];
                res[i] = r;
                m[r_g + i] = (uint64_t)(uintptr_t)(stored ? d_in + b.src_off : d_tmp + ci * B);
                m[r_g + nb + i] = pos;
                m[r_g + 2 * nb + i] = r > 0 ? (uint64_t)r : 0;
                if (r > 0) pos += (uint64_t)r;
                if (!stored) ci++;
            }
            if (!e->d_out.reserve(pos + 16)) return CJ_E_OOM;
            d_final = (uint8_t*)e->d_out.p;
            HIP_TRY(hipMemcpyAsync(d_meta + r_g, m.data() + r_g, 3 * nb * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
            cj::launch_copy_segments(d_meta + r_g, d_final, d_meta + r_g + nb, d_meta + r_g + 2 * nb, nullptr, 0, (uint32_t)nb, s);
            HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
        } else if (B == 65536 && !lz4f_chain_only() && lz4_frame_linked_lds(e, f, d_in, res, &d_final) == 0) {
            // linked 64 KiB blocks, decoded by the two-window LDS workgroup decoder (results in res, bytes at d_final)
        } else {
            // linked blocks: the chain kernel decodes straight into the contiguous output
            const uint64_t out_cap = nb * B;
            const size_t words = (nb * 4 + 7) / 8, rows = nb + words + nb;      // blk_off | word (u32) | result
            if (!e->d_out.reserve(out_cap + 16) || !e->d_meta.reserve(rows * 8)) return CJ_E_OOM;
            d_final = (uint8_t*)e->d_out.p;
            uint64_t* d_meta = (uint64_t*)e->d_meta.p;
            std::vector<uint64_t>& m = e->h_meta;
            m.assign(rows, 0);
            uint32_t* wv = reinterpret_cast<uint32_t*>(m.data() + nb);
            for (size_t i = 0; i < nb; i++) { m[i] = f.blocks[i].src_off; wv[i] = f.blocks[i].word; }
            HIP_TRY(hipMemcpyAsync(d_meta, m.data(), (nb + words) * 8, hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
            cj::launch_lz4_frame_chain(d_in, d_meta, (const uint32_t*)(d_meta + nb), (uint32_t)nb, d_final, out_cap, (uint32_t)B,
                                       (int64_t*)(d_meta + nb + words), s);
            HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
            HIP_TRY(hipMemcpyAsync(res.data(), d_meta + nb + words, nb * 8, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
            HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
        }
        // first failure in stream order: malformed block, then the writer running out of room
        for (size_t i = 0; i < nb; i++) {
            if (res[i] < 0) return CJ_E_LZ4F_DECOMPRESS;
            if (f.csize && total + (uint64_t)res[i] > f.content_size) return CJ_E_LZ4F_CONTENT_SIZE;      // more than the header announced (LZ4F: ERROR_frameSize_wrong)
            if (out != nullptr && total + (uint64_t)res[i] > cap) return CJ_E_FRAME_WRITE;
            total += (uint64_t)res[i];
        }
        if (out != nullptr && total) {
            HIP_TRY(hipMemcpyAsync(out, d_final, total, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
            HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
        }
    }
    if (f.late_err && !f.complete) return f.late_err;                      // truncated / bad block word or checksum: after the blocks before it
    if (f.csize && f.content_size != total) return CJ_E_LZ4F_CONTENT_SIZE;
    if (f.late_err) return f.late_err;                                       // content checksum word missing
    if (f.csum && out != nullptr && f.content_sum != xxh32(out, total, 0)) return CJ_E_LZ4F_CONTENT_CHECKSUM;
    return (int64_t)total;
}

}  // extern "C"
