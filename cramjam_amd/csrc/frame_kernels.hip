// frame_kernels.hip — device side of the framed formats (frame.hip, frame_batch.hip): per-piece CRC-32C and the segment
// mover that assembles / unpacks a framed stream in HBM (one wavefront per piece or segment, 4 per block); for batches of
// streams the grammar walk (one lane per stream, frame_grammar.hpp), XXH32 (one wavefront per stream), the stream-order verdict
// with the compaction of the decoded blocks and the assembly of compressed frames (one wavefront per stream).
#include "cj_stage.hpp"
#include "crc32c_lanes.hpp"
#include "frame_grammar.hpp"

namespace cj {

namespace {
__device__ const Crc32cTables d_crc_tables = make_crc32c_tables();
}

// out[i] = masked CRC-32C of base[off[i] .. off[i] + len[i])      (framing_format.txt §3; len < 2^32)
__global__ __launch_bounds__(kBlockThreads) void crc32c_pieces_kernel(const uint8_t* base, const uint64_t* off,
                                                                      const uint64_t* len, uint32_t* out, uint32_t n) {
    __shared__ uint32_t adv[1024];
    for (uint32_t i = threadIdx.x; i < 1024u; i += kBlockThreads) adv[i] = (&d_crc_tables.adv256[0][0])[i];
    __syncthreads();
    const uint32_t piece = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (piece >= n) return;
    uint32_t c = crc32c_lane(base + off[piece], (uint32_t)len[piece], lane_id(), adv, d_crc_tables.xpow8,
                             [](const uint8_t* p) { return ld32u(p); });
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) c ^= __shfl_xor(c, sh, 64);
    if (lane_id() == 0) out[piece] = crc32c_mask(~c);
}

// segment i: len[i] bytes from the device address src[i] to dst_base + dst_off[i]; when hdr is non-null the low
// hdr_len (<= 8) bytes of hdr[i], little endian, are written just before the segment (Snappy: chunk type, u24 length,
// u32 checksum; LZ4 frame: u32 block size word).
__global__ __launch_bounds__(kBlockThreads) void copy_segments_kernel(const uint64_t* src, uint8_t* dst_base,
                                                                      const uint64_t* dst_off, const uint64_t* len,
                                                                      const uint64_t* hdr, uint32_t hdr_len, uint32_t n) {
    const uint32_t seg = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (seg >= n) return;
    uint8_t* dst = dst_base + dst_off[seg];
    if (hdr != nullptr) {
        const uint64_t h = hdr[seg];
        if (lane_id() < hdr_len) dst[(int)lane_id() - (int)hdr_len] = (uint8_t)(h >> (8u * lane_id()));
    }
    wave_copy(dst, reinterpret_cast<const uint8_t*>(src[seg]), (uint32_t)len[seg]);
}

void launch_crc32c_pieces(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint32_t* out, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(crc32c_pieces_kernel, dim3((n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlockThreads), 0, s, base, off, len, out, n);
}

void launch_copy_segments(const uint64_t* src, uint8_t* dst_base, const uint64_t* dst_off, const uint64_t* len,
                          const uint64_t* hdr, uint32_t hdr_len, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(copy_segments_kernel, dim3((n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlockThreads), 0, s, src, dst_base, dst_off, len, hdr, hdr_len, n);
}

// ---- batches of framed streams ------------------------------------------------------------------------------------------

__device__ __forceinline__ void wave_copy64(uint8_t* dst, const uint8_t* src, uint64_t n) {
    for (uint64_t o = 0; o < n; o += (1u << 30)) wave_copy(dst + o, src + o, (uint32_t)(n - o < (1u << 30) ? n - o : (1u << 30)));
}

// (lz4_slot_bytes, the scratch of one LZ4 block: frame_grammar.hpp)
__global__ __launch_bounds__(kBlockThreads) void fb_walk_kernel(int fmt, uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                const uint64_t* in_len, uint64_t* cnt, FbFrame* fr, FbRows r,
                                                                ChainJob* jobs) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t* in = in_base + in_off[i];
    const size_t len = (size_t)in_len[i];
    if (fmt == CJ_FORMAT_SNAPPY_FRAMED) {
        uint64_t total = 0;
        if (cnt) {
            uint32_t nb = 0;
            snappy_frame_walk(in, len, [&](const SnapPiece&) { nb++; }, &total);
            cnt[2 * i] = nb; cnt[2 * i + 1] = total;
            return;
        }
        FbFrame f = fr[i];
        uint64_t g = f.blk0;
        f.late = snappy_frame_walk(in, len, [&](const SnapPiece& p) {
            const uint64_t at = in_off[i] + p.src_off, dst = f.slot0 + p.dst_off;
            r.b.in_off[g] = at; r.b.in_len[g] = p.stored ? 0 : p.src_len;
            r.b.out_off[g] = dst; r.b.out_cap[g] = p.stored ? 0 : p.dst_len;
            r.cp_src[g] = (uint64_t)(uintptr_t)(in_base + at); r.cp_dst[g] = dst; r.cp_len[g] = p.stored ? p.dst_len : 0;
            r.ck_off[g] = dst; r.ck_len[g] = p.dst_len;
            r.word[g] = p.dst_len | (p.stored ? 0x80000000u : 0u); r.expect[g] = p.crc;
            g++;
        }, &total);
        f.err = 0; f.total = total;
        fr[i] = f;
        return;
    }
    Lz4Header h;
    if (cnt) {
        uint32_t nb = 0;
        uint64_t slots = 0, chain = 0;                               // scratch of independent slots / of a linked frame's contiguous output
        const int64_t err = lz4_frame_walk(in, len, h, [&](uint64_t, uint32_t w) {
            nb++;
            const uint64_t b = lz4_slot_bytes(w, h.block_max);
            chain += b;
            if (!(w & 0x80000000u)) slots += up16(b);
            return true;
        });
        if (err || h.skippable) nb = 0;
        cnt[2 * i] = nb; cnt[2 * i + 1] = nb == 0 ? 0 : (!h.indep && nb > 1) ? chain : slots;
        return;
    }
    FbFrame f = fr[i];
    const bool linked = f.nblk > 1;                                   // (set below once the header is known)
    uint64_t g = f.blk0, at = f.slot0, chain = 0;
    f.err = lz4_frame_walk(in, len, h, [&](uint64_t pos, uint32_t w) {
        const uint32_t sz = w & 0x7FFFFFFFu;
        const bool skip = (w & 0x80000000u) || (linked && !h.indep);   // stored blocks: the finisher copies them; linked: the chain kernel
        const uint64_t b = lz4_slot_bytes(w, h.block_max);
        r.b.in_off[g] = in_off[i] + pos; r.b.in_len[g] = skip ? 0 : sz;
        r.b.out_off[g] = skip ? 0 : at; r.b.out_cap[g] = skip ? 0 : b;
        if (!skip) at += up16(b);
        chain += b;
        r.ck_off[g] = in_off[i] + pos; r.ck_len[g] = h.bsum ? sz : 0;
        r.word[g] = w; r.expect[g] = h.bsum ? fg_rd32(in + pos + sz) : 0u;
        g++;
        return true;
    });
    f.late = h.late_err; f.content_size = h.content_size; f.content_sum = h.content_sum; f.block_max = h.block_max;
    f.bits = (h.indep ? kFbIndep : 0) | (h.bsum ? kFbBsum : 0) | (h.csize ? kFbCsize : 0) | (h.csum ? kFbCsum : 0) |
             (h.skippable ? kFbSkip : 0) | (h.complete ? kFbComplete : 0);
    fr[i] = f;
    ChainJob j = {};
    if (f.err == 0 && !h.skippable && linked && !h.indep) j = { f.blk0, f.slot0, chain, f.nblk, h.block_max };
    jobs[i] = j;
}

void launch_fb_walk(int fmt, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint64_t* cnt,
                    FbFrame* fr, FbRows r, ChainJob* jobs, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fb_walk_kernel, dim3((uint32_t)((n + kBlockThreads - 1) / kBlockThreads)), dim3(kBlockThreads), 0, s,
                       fmt, (uint32_t)n, in_base, in_off, in_len, cnt, fr, r, jobs);
}

// XXH32 of p[0, n) by one wavefront (the result is uniform).  The stream is read as the aligned 16-byte granules that hold it (never
// past the granule of its last byte); lane l cuts stripe i0 + l out of two granules by byte shifts, so a wavefront fetches 1 KiB per
// step, coalesced, and the next KiB's loads are in flight while the recurrence — four dependent multiply-rotate chains, serial by
// definition — reads this KiB's 64 stripes lane by lane (readlane).
__device__ __forceinline__ uint32_t xx_round(uint32_t v, uint32_t w) { return fg_rotl(v + w * 2246822519u, 13) * 2654435761u; }

__device__ __forceinline__ uint4 xx_cut(uint4 a, uint4 b, uint32_t q, uint32_t sh) {
    const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    uint32_t u[5];
#pragma unroll
    for (int k = 0; k < 5; k++) u[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
    return make_uint4(__builtin_amdgcn_alignbit(u[1], u[0], sh), __builtin_amdgcn_alignbit(u[2], u[1], sh),
                      __builtin_amdgcn_alignbit(u[3], u[2], sh), __builtin_amdgcn_alignbit(u[4], u[3], sh));
}

__device__ uint32_t xxh32_wave(const uint8_t* p, uint64_t n) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint64_t ns = n / 16;
    uint32_t h;
    if (ns) {
        uint32_t v0 = P1 + P2, v1 = P2, v2 = 0u, v3 = 0u - P1;
        const uint32_t mis = (uint32_t)((uintptr_t)p & 15u), q = mis >> 2, sh = (mis & 3u) * 8u;
        const uint4* g = reinterpret_cast<const uint4*>(p - mis);
        const auto fetch = [&](uint64_t i0, uint4& a, uint4& b) {
            const uint64_t i = i0 + lane_id();
            a = make_uint4(0, 0, 0, 0); b = a;
            if (i < ns) { a = g[i]; b = mis ? g[i + 1] : a; }   // (the granule after stripe i holds stream bytes only when misaligned)
        };
        uint4 a, b;
        fetch(0, a, b);
        for (uint64_t i0 = 0; i0 < ns; i0 += 64) {
            const uint4 w = xx_cut(a, b, q, sh);
            if (i0 + 64 < ns) fetch(i0 + 64, a, b);
            const uint32_t m = (uint32_t)(ns - i0 < 64 ? ns - i0 : 64);
            if (m == 64) {
#pragma unroll
                for (uint32_t j = 0; j < 64; j++) {
                    v0 = xx_round(v0, rdlane(w.x, j)); v1 = xx_round(v1, rdlane(w.y, j));
                    v2 = xx_round(v2, rdlane(w.z, j)); v3 = xx_round(v3, rdlane(w.w, j));
                }
            } else {
                for (uint32_t j = 0; j < m; j++) {
                    v0 = xx_round(v0, rdlane(w.x, j)); v1 = xx_round(v1, rdlane(w.y, j));
                    v2 = xx_round(v2, rdlane(w.z, j)); v3 = xx_round(v3, rdlane(w.w, j));
                }
            }
        }
        h = fg_rotl(v0, 1) + fg_rotl(v1, 7) + fg_rotl(v2, 12) + fg_rotl(v3, 18);
    } else {
        h = P5;
    }
    h += (uint32_t)n;
    const uint8_t* t = p + ns * 16;
    uint32_t k = 0;
    const uint32_t nt = (uint32_t)(n - ns * 16);
    for (; k + 4 <= nt; k += 4) h = fg_rotl(h + fg_rd32(t + k) * P3, 17) * P4;
    for (; k < nt; k++) h = fg_rotl(h + (uint32_t)t[k] * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// out[i] = XXH32(base + off[i] .. + len[i]), one wavefront per stream
__global__ __launch_bounds__(kBlockThreads) void xxh32_streams_kernel(const uint8_t* base, const uint64_t* off, const uint64_t* len,
                                                                      uint32_t* out, uint32_t n) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const uint32_t h = xxh32_wave(base + off[i], len[i]);
    if (lane_id() == 0) out[i] = h;
}

void launch_xxh32_streams(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint32_t* out, size_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(xxh32_streams_kernel, dim3((uint32_t)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlockThreads), 0, s,
                       base, off, len, out, (uint32_t)n);
}

// LZ4: the verdict of cj_lz4_frame_decompress for each frame (frame.hip), block results from the engine / the chain kernel, block
// checksums from xxh32_streams; the decoded blocks (slots of block_max in the scratch, stored blocks in the stream) compacted
// into the caller's slot.  Snappy: cj_snappy_frame_decompress's order; the pieces lie decoded back to back in the scratch.
__global__ __launch_bounds__(kBlockThreads) void fb_finish_kernel(int fmt, uint32_t n, const FbFrame* fr, FbRows r, const uint8_t* in_base,
                                                                  const uint8_t* scratch, uint8_t* out_base, const uint64_t* out_off,
                                                                  const uint64_t* out_cap, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const FbFrame f = fr[i];
    const uint64_t cap = out_cap[i];
    uint8_t* dst = out_base + out_off[i];
    int64_t res = 0;
    if (fmt == CJ_FORMAT_SNAPPY_FRAMED) {
        uint64_t written = 0;
        for (uint32_t k = 0; k < f.nblk && res == 0; k++) {
            const uint64_t g = f.blk0 + k;
            const uint32_t w = uni(r.word[g]);
            if (!(w & 0x80000000u) && r.b.result[g] < 0) res = r.b.result[g];
            else if (r.got[g] != r.expect[g]) res = CJ_E_SNAPPY_CHECKSUM;
            else if (written + (w & 0x7FFFFFFFu) > cap) res = CJ_E_FRAME_WRITE;
            written += w & 0x7FFFFFFFu;
        }
        if (res == 0 && f.late) res = f.late;
        if (res == 0) {
            wave_copy64(dst, scratch + f.slot0, f.total);
            res = (int64_t)f.total;
        }
        if (lane_id() == 0) result[i] = res;
        return;
    }
    if (f.err || (f.bits & kFbSkip)) {
        if (lane_id() == 0) result[i] = f.err;
        return;
    }
    uint32_t nb = f.nblk;
    int64_t late = f.late;
    bool complete = (f.bits & kFbComplete) != 0;
    if (f.bits & kFbBsum)                                    // (the host walk stops at the first bad block checksum)
        for (uint32_t k = 0; k < nb; k++)
            if (r.got[f.blk0 + k] != r.expect[f.blk0 + k]) { nb = k; late = CJ_E_LZ4F_BLOCK_CHECKSUM; complete = false; break; }
    const uint64_t B = f.block_max;
    const bool chained = !(f.bits & kFbIndep) && f.nblk > 1;
    // (frame.hip takes independent blocks above 64 KiB through the large-stream path when they surely fit: no size or room checks
    //  between the blocks there)
    uint64_t bound = 0;
    for (uint32_t k = 0; k < nb; k++) { const uint32_t w = r.word[f.blk0 + k]; bound += (w & 0x80000000u) ? (w & 0x7FFFFFFFu) : B; }
    const bool big = B > 65536 && (f.bits & kFbIndep) && nb > 0 && bound <= cap;
    const bool csize = (f.bits & kFbCsize) != 0;
    uint64_t total = 0;
    for (uint32_t k = 0; k < nb && res == 0; k++) {
        const uint64_t g = f.blk0 + k;
        const uint32_t w = uni(r.word[g]);
        const int64_t rk = ((w & 0x80000000u) && !chained) ? (int64_t)(w & 0x7FFFFFFFu) : r.b.result[g];
        if (rk < 0) { res = CJ_E_LZ4F_DECOMPRESS; break; }
        if (!big && csize && total + (uint64_t)rk > f.content_size) { res = CJ_E_LZ4F_CONTENT_SIZE; break; }
        if (!big && total + (uint64_t)rk > cap) { res = CJ_E_FRAME_WRITE; break; }
        total += (uint64_t)rk;
    }
    if (res == 0 && late && !complete) res = late;
    if (res == 0 && csize && f.content_size != total) res = CJ_E_LZ4F_CONTENT_SIZE;
    if (res == 0 && late) res = late;
    if (res == 0) {
        if (chained) wave_copy64(dst, scratch + f.slot0, total);
        else {
            uint64_t pos = 0;
            for (uint32_t k = 0; k < nb; k++) {
                const uint64_t g = f.blk0 + k;
                const uint32_t w = uni(r.word[g]);
                const bool stored = (w & 0x80000000u) != 0;
                const uint32_t rk = stored ? (w & 0x7FFFFFFFu) : (uint32_t)r.b.result[g];
                wave_copy(dst + pos, stored ? in_base + r.b.in_off[g] : scratch + r.b.out_off[g], rk);
                pos += rk;
            }
        }
        res = (int64_t)total;
    }
    if (lane_id() == 0) result[i] = res;
}

// LZ4: the content checksum over what fb_finish_kernel wrote, one wavefront per frame
__global__ __launch_bounds__(kBlockThreads) void fb_content_sum_kernel(uint32_t n, const FbFrame* fr, const uint8_t* out_base,
                                                                       const uint64_t* out_off, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const int64_t r = result[i];
    if (r < 0 || fr[i].err || !(fr[i].bits & kFbCsum) || (fr[i].bits & kFbSkip)) return;
    const uint32_t h = xxh32_wave(out_base + out_off[i], (uint64_t)r);
    if (lane_id() == 0 && h != fr[i].content_sum) result[i] = CJ_E_LZ4F_CONTENT_CHECKSUM;
}

void launch_fb_finish(int fmt, size_t n, const FbFrame* fr, FbRows r, const uint8_t* in_base, const uint8_t* scratch, uint8_t* out_base,
                      const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fb_finish_kernel, dim3((uint32_t)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlockThreads), 0, s,
                       fmt, (uint32_t)n, fr, r, in_base, scratch, out_base, out_off, out_cap, result);
    if (fmt == CJ_FORMAT_LZ4_FRAME)
        hipLaunchKernelGGL(fb_content_sum_kernel, dim3((uint32_t)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlockThreads), 0, s,
                           (uint32_t)n, fr, out_base, out_off, result);
}

__global__ __launch_bounds__(kBlockThreads) void fb_pieces_kernel(uint32_t n, const FbFrame* fr, const uint64_t* in_off, const uint64_t* in_len,
                                                                  BatchRows b, uint64_t stride) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = in_len[i], p0 = fr[i].blk0;
    for (uint32_t k = 0; k < fr[i].nblk; k++) {
        const uint64_t g = p0 + k, at = (uint64_t)k * kSnapPiece;
        b.in_off[g] = in_off[i] + at;
        b.in_len[g] = len - at < kSnapPiece ? len - at : kSnapPiece;
        b.out_off[g] = g * stride;
        b.out_cap[g] = stride;
    }
}

void launch_fb_pieces(size_t n, const FbFrame* fr, const uint64_t* in_off, const uint64_t* in_len, BatchRows b, uint64_t stride, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fb_pieces_kernel, dim3((uint32_t)((n + kBlockThreads - 1) / kBlockThreads)), dim3(kBlockThreads), 0, s,
                       (uint32_t)n, fr, in_off, in_len, b, stride);
}

// the low `bytes` (<= 8) bytes of v, little endian, at p (one lane each)
__device__ __forceinline__ void wave_put(uint8_t* p, uint64_t v, uint32_t bytes) {
    if (lane_id() < bytes) p[lane_id()] = (uint8_t)(v >> (8u * lane_id()));
}

// The single-call compressors' layout (frame.hip): LZ4 FLG 0x64 / BD 0x40, a block is stored when it does not shrink; Snappy: the stream
// identifier, a chunk is stored when compressed >= len - len / 8.  Nothing is written unless the whole frame fits out_cap.
__global__ __launch_bounds__(kBlockThreads) void fb_assemble_kernel(int fmt, uint32_t n, const FbFrame* fr, FbRows r, const uint32_t* sums,
                                                                    const uint8_t* in_base, const uint64_t* in_len,
                                                                    const uint8_t* scratch, uint64_t stride, uint8_t* out_base,
                                                                    const uint64_t* out_off, const uint64_t* out_cap, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const bool lz4 = fmt == CJ_FORMAT_LZ4_FRAME;
    const uint64_t cap = out_cap[i], len = in_len[i], p0 = fr[i].blk0;
    const uint32_t np = uni(fr[i].nblk);
    int64_t res = 0;
    if (lz4 && cap < 15) res = CJ_E_FRAME_WRITE;
    else if (!lz4 && len == 0) res = 0;
    else {
        uint64_t total = lz4 ? 15 : 10;
        for (uint32_t k = 0; k < np && res == 0; k++) {
            const int64_t c = r.b.result[p0 + k];
            const uint64_t l = r.b.in_len[p0 + k];
            if (c < 0) { res = c; break; }
            const bool stored = lz4 ? (uint64_t)c >= l : (uint64_t)c >= l - l / 8;
            total += (lz4 ? 4 : 8) + (stored ? l : (uint64_t)c);
        }
        if (res == 0 && total > cap) res = CJ_E_FRAME_WRITE;
        if (res == 0) {
            uint8_t* dst = out_base + out_off[i];
            uint64_t pos;
            if (lz4) {
                const uint8_t fd[2] = { 0x64, 0x40 };
                wave_put(dst, 0x184D2204ull | (0x64ull << 32) | (0x40ull << 40) | ((uint64_t)(uint8_t)(xxh32_short(fd, 2) >> 8) << 48), 7);
                pos = 7;
            } else {
                wave_put(dst, 0x50614e73000006ffull, 8);                                             /* ff 06 00 00 's' 'N' 'a' 'P' */
                wave_put(dst + 8, 0x5970ull, 2);                                                       /* 'p' 'Y' */
                pos = 10;
            }
            for (uint32_t k = 0; k < np; k++) {
                const uint64_t g = p0 + k, l = r.b.in_len[g], c = (uint64_t)r.b.result[g];
                const bool stored = lz4 ? c >= l : c >= l - l / 8;
                const uint64_t body = stored ? l : c;
                if (lz4) { wave_put(dst + pos, body | (stored ? 0x80000000ull : 0ull), 4); pos += 4; }
                else { wave_put(dst + pos, (stored ? 1ull : 0ull) | ((body + 4) << 8) | ((uint64_t)r.got[g] << 32), 8); pos += 8; }
                wave_copy(dst + pos, stored ? in_base + r.b.in_off[g] : scratch + g * stride, (uint32_t)body);
                pos += body;
            }
            if (lz4) wave_put(dst + pos, (uint64_t)sums[i] << 32, 8);                      // EndMark, content checksum
            res = (int64_t)total;
        }
    }
    if (lane_id() == 0) result[i] = res;
}

void launch_fb_assemble(int fmt, size_t n, const FbFrame* fr, FbRows r, const uint32_t* sums, const uint8_t* in_base, const uint64_t* in_len, const uint8_t* scratch, uint64_t stride, uint8_t* out_base, const uint64_t* out_off,
                        const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fb_assemble_kernel, dim3((uint32_t)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlockThreads), 0, s,
                       fmt, (uint32_t)n, fr, r, sums, in_base, in_len, scratch, stride, out_base, out_off, out_cap, result);
}

}  // namespace cj
