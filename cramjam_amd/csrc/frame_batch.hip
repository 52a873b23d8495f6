// frame_batch.hip — many independent framed streams per call (cj_frame_batch_device / cj_frame_batch_host): LZ4 frames and
// Snappy framed streams, both directions.  Everything specific to the format runs on the device, because a device batch has no
// host copy of its streams: the grammar walk (one lane per stream, two passes around one read-back of the block counts), XXH32
// and CRC-32C, the stream-order verdict and the assembly (frame_kernels.hip).  The blocks go through the batch engine as one
// batch; linked LZ4 blocks through the chain kernel, one wavefront per frame.  The verdicts are those of the single-stream
// exports in frame.hip.
#include "cj_stage.hpp"

namespace {

constexpr uint64_t kLz4Stride = 65824;       // LZ4_compressBound(65536) = 65809, rounded up to 16
constexpr uint64_t kSnapStride = 76496;      // max_compress_len(65536) = 76490, rounded up to 16
constexpr uint64_t kPiece = 65536;

using cj::up16;

int frame_batch(cj_engine* e, cj_format fmt, cj_op op, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch (e->d_fb, e->h_fb: frame batches and Blosc chunk batches).  The lock is held across the
    // call's one wait: such batches on one engine run one after another, and a call waits for everything its caller queued on `s` before
    // it, so a second caller's batch also waits behind that (engines are cheap: one per thread or stream avoids it).
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    const size_t tab = up16(n * sizeof(cj::FbFrame));
    int rc;
    if ((rc = turn.reserve(e->d_fb, std::max(16 * n, tab))) != 0 || (rc = turn.reserve(e->h_fb, tab + 16 * n)) != 0) return rc;
    uint64_t* cnt = (uint64_t*)e->h_fb.p;                                         // read back: [2i] blocks, [2i + 1] scratch bytes / in_len
    cj::FbFrame* h_fr = reinterpret_cast<cj::FbFrame*>(e->h_fb.p + 16 * n);
    const bool dec = op == CJ_OP_DECOMPRESS;
    // the one wait: the host sizes the block rows and the scratch from the streams' block counts (decompress) / lengths (compress)
    if (dec) {
        cj::launch_fb_walk(fmt, n, in_base, in_off, in_len, (uint64_t*)e->d_fb.p, nullptr, cj::FbRows{}, nullptr, s);
        HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
        HIP_TRY(hipMemcpyAsync(cnt, e->d_fb.p, 16 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    } else {
        HIP_TRY(hipMemcpyAsync(cnt, in_len, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    }
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    std::memset(h_fr, 0, n * sizeof(cj::FbFrame));
    uint64_t nb = 0, slot = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = dec ? cnt[2 * i] : (cnt[i] + kPiece - 1) / kPiece;
        h_fr[i].blk0 = nb; h_fr[i].slot0 = slot; h_fr[i].nblk = (uint32_t)k;
        nb += k;
        if (dec) slot += up16(cnt[2 * i + 1]);
    }
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    const uint64_t stride = fmt == CJ_FORMAT_LZ4_FRAME ? kLz4Stride : kSnapStride;
    if (!dec) slot = nb * stride;
    // d_fb: frames | chain jobs (decompress) / content sums (compress) | block rows | scratch
    const size_t o_side = tab, o_rows = o_side + up16(n * sizeof(cj::ChainJob)), o_scr = o_rows + cj::kFbRowWords * 8 * nb;
    if ((rc = turn.reserve(e->d_fb, o_scr + slot + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    cj::FbFrame* fr = reinterpret_cast<cj::FbFrame*>(d);
    const cj::FbRows r = cj::fb_rows(reinterpret_cast<uint64_t*>(d + o_rows), nb);
    uint8_t* scratch = d + o_scr;
    HIP_TRY(hipMemcpyAsync(fr, h_fr, n * sizeof(cj::FbFrame), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    if (dec) {
        cj::ChainJob* jobs = reinterpret_cast<cj::ChainJob*>(d + o_side);
        cj::launch_fb_walk(fmt, n, in_base, in_off, in_len, nullptr, fr, r, jobs, s);
        if (nb) {
            cj::BatchArgs a;
            cj::fill_args(a, 0, in_base, scratch, r.b);
            rc = cj::launch(e, fmt == CJ_FORMAT_LZ4_FRAME ? CJ_CODEC_LZ4_BLOCK : CJ_CODEC_SNAPPY_RAW, CJ_OP_DECOMPRESS, a, s);
            if (rc != 0) return rc;
        }
        if (fmt == CJ_FORMAT_LZ4_FRAME) {
            cj::launch_lz4_frame_chains(in_base, r.b.in_off, r.word, scratch, r.b.result, jobs, (uint32_t)n, s);
            cj::launch_xxh32_streams(in_base, r.ck_off, r.ck_len, r.got, nb, s);
        } else {
            cj::launch_copy_segments(r.cp_src, scratch, r.cp_dst, r.cp_len, nullptr, 0, (uint32_t)nb, s);
            cj::launch_crc32c_pieces(scratch, r.ck_off, r.ck_len, r.got, (uint32_t)nb, s);
        }
        cj::launch_fb_finish(fmt, n, fr, r, in_base, scratch, out_base, out_off, out_cap, result, s);
    } else {
        uint32_t* sums = reinterpret_cast<uint32_t*>(d + o_side);
        cj::launch_fb_pieces(n, fr, in_off, in_len, r.b, stride, s);
        if (nb) {
            cj::BatchArgs a;
            cj::fill_args(a, 0, in_base, scratch, r.b);
            rc = cj::launch(e, fmt == CJ_FORMAT_LZ4_FRAME ? CJ_CODEC_LZ4_BLOCK : CJ_CODEC_SNAPPY_RAW, CJ_OP_COMPRESS, a, s);
            if (rc != 0) return rc;
        }
        if (fmt == CJ_FORMAT_LZ4_FRAME) cj::launch_xxh32_streams(in_base, in_off, in_len, sums, n, s);
        else cj::launch_crc32c_pieces(in_base, r.b.in_off, r.b.in_len, r.got, (uint32_t)nb, s);
        cj::launch_fb_assemble(fmt, n, fr, r, sums, in_base, in_len, scratch, stride, out_base, out_off, out_cap, result, s);
    }
    return turn.done(s);
}

bool fb_args_ok(cj_engine* e, cj_format fmt, cj_op op, uint32_t flags) {
    return e && flags == 0 && (fmt == CJ_FORMAT_LZ4_FRAME || fmt == CJ_FORMAT_SNAPPY_FRAMED) && (op == CJ_OP_DECOMPRESS || op == CJ_OP_COMPRESS);
}

}  // namespace

extern "C" {

int cj_frame_batch_device(cj_engine* e, cj_format fmt, cj_op op, uint32_t flags, size_t n_frames,
                          const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                          uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                          int64_t* result, void* hip_stream) {
    if (!fb_args_ok(e, fmt, op, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_frames, {}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return frame_batch(e, fmt, op, n_frames, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_frame_batch_host(cj_engine* e, cj_format fmt, cj_op op, uint32_t flags, size_t n,
                        const uint8_t* const* in_ptrs, const size_t* in_lens,
                        uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!fb_args_ok(e, fmt, op, flags)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine*, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return frame_batch(e, fmt, op, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

// debug aid (tests): XXH32 of n device streams by the batch's kernel, on the engine's stream, synchronously
int cj_debug_xxh32_device(cj_engine* e, const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len, uint32_t* d_out, size_t n) {
    if (!e) return CJ_E_BAD_ARG;
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    cj::launch_xxh32_streams(d_base, d_off, d_len, d_out, n, e->stream);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    return 0;
}

}  // extern "C"
