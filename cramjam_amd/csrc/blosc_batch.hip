// blosc_batch.hip — batches of Blosc chunks (cj_blosc_batch_device / _host), their size query and the single-chunk exports on top.
// Shaped like frame_batch.hip: everything specific to the container runs on the device, because a device batch has no host copy.
//   decompress  walk pass 1 (one lane per chunk: streams, blocks, scratch) -> the one wait (prefix sums on the host) -> walk pass 2
//               (stream rows, filter block rows) -> the LZ4 streams of all chunks through the engine: those of transposed blocks as
//               one batch into the scratch, those of blocks that need no transposition (no filter, typesize 1 under shuffle,
//               bitshuffle's odd blocks) as one batch straight into the callers' slots — no scratch, no second pass; the BloscLZ
//               streams (CJ_BLOSC_FLAG_READ_BLOSCLZ) the same two ways through blosclz_decode.hip, the Zlib and Zstd streams
//               (CJ_BLOSC_FLAG_READ_ZLIB / _ZSTD) through the launchers of deflate.hip and zstd.hip; stored streams
//               by copy_segments likewise -> the verdict (one lane per chunk) -> ONE unfilter launch from the scratch into the
//               callers' slots (blocks of a chunk with an error are skipped)
//   compress    in_len read back -> rows -> ONE filter launch into the scratch (transposed blocks only) -> the engine over all
//               streams (from the scratch / straight from the input) -> one wavefront per chunk assembles header, bstarts, stream
//               words and payloads (or the memcpyed chunk)
// The grammar is blosc_grammar.hpp's, the transpositions blosc_filters.hip's.
#include "blosc_filters.hpp"
#include "cj_codecs.hpp"

namespace cj {

// pass 1 of the decode walk, read back by the host.  A stream is DIRECT when its block needs no transposition (blosc_block_mode ==
// kBloscCopy): it decodes straight into the caller's slot; every other stream decodes into the scratch, which the unfilter launch reads
struct BlCount { uint32_t nstr, ndir, nblk, nbytes, scratch, maxlen, tiles, format; int64_t err; };   // nblk: filtered blocks (memcpyed: copy pieces); format: kBloscFormat* of the streams
// one row per chunk: where its streams (scratch / direct), filter blocks and scratch begin (host prefix sums)
struct BlChunk { uint64_t strm0, dstrm0, blk0, slot0, cslot0; int64_t err; uint32_t nstr, ndir, nblk, nbytes; };
// the per-stream rows are CopyRows (cj_codecs.hpp): the engine's batch and the stored streams' copy_segments rows; rows [0, na) are the
// scratch streams of all chunks, behind them the direct ones; either half is ordered by format — LZ4 | BloscLZ | Zlib | Zstd
// (bl_class) —, and the streams of a chunk, which all have its one format, lie together

// the row range of a chunk's streams by its compressor format: 0 LZ4 (and every chunk without streams), 1 BloscLZ, 2 Zlib, 3 Zstd
constexpr int kBlClasses = 4;
inline int bl_class(uint32_t format) {
    return format == kBloscFormatBlosclz ? 1 : format == kBloscFormatZlib ? 2 : format == kBloscFormatZstd ? 3 : 0;
}
constexpr Inner bl_inner(int cls) { return cls == 1 ? kInBloscLz : cls == 2 ? kInZlib : cls == 3 ? kInZstd : kInLz4Raw; }

constexpr uint32_t kMemcpyPiece = 1u << 20;          // a memcpyed chunk goes through the filter launch as copy rows of this size
// room the LZ4 encoder asks for a stream of n bytes (lz4_encode.hip), rounded up to 16
__host__ __device__ inline uint64_t bl_enc_room(uint32_t n) { return up16((uint64_t)n + n / 255u + 16u); }
__host__ __device__ inline uint32_t bl_block_bytes(uint32_t nbytes, uint32_t blocksize, uint32_t b) {
    const uint32_t at = b * blocksize;
    return nbytes - at < blocksize ? nbytes - at : blocksize;
}

__global__ __launch_bounds__(kBlockThreads) void bl_walk_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                                                BlCount* cnt, const BlChunk* tab, CopyRows r, BloscBlockRow* blocks, uint8_t* scratch, uint32_t rflags) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t* in = in_base + in_off[i];
    const size_t len = (size_t)in_len[i];
    BloscHeader h;
    const auto direct = [&](uint32_t b) { return blosc_block_mode(h.flags, h.typesize, bl_block_bytes(h.nbytes, h.blocksize, b)) == kBloscCopy; };
    if (cnt) {
        BlCount c = {};
        c.err = blosc_walk(in, len, h, [&](const BloscStream& s) {
            if (direct(s.block)) c.ndir++; else c.nstr++;
            if (!s.stored && s.dst_len > c.maxlen) c.maxlen = s.dst_len;
        }, rflags);
        if (c.err == 0 && h.nbytes > out_cap[i]) c.err = CJ_E_OUT_TOO_SMALL;
        c.nbytes = h.nbytes; c.format = h.format;
        if (c.err != 0 || h.nbytes == 0) { c.nstr = 0; c.ndir = 0; c.maxlen = 0; }
        else if (h.flags & kBloscMemcpyed) { c.nblk = (h.nbytes + kMemcpyPiece - 1) / kMemcpyPiece; c.tiles = kMemcpyPiece / kBloscTileBytes; }
        else {
            for (uint32_t b = 0; b < h.nblocks; b++) c.nblk += direct(b) ? 0u : 1u;
            if (c.nblk) { c.scratch = 1; c.tiles = blosc_tiles(h.typesize, h.blocksize); }
        }
        cnt[i] = c;
        return;
    }
    const BlChunk ch = tab[i];
    if (ch.err != 0 || ch.nstr + ch.ndir + ch.nblk == 0) return;
    if (blosc_header(in, len, h, rflags) != 0) return;                // (pass 1 accepted it: cannot happen)
    uint8_t* dst = out_base + out_off[i];
    if (h.flags & kBloscMemcpyed) {
        for (uint32_t k = 0; k < ch.nblk; k++) {
            const uint32_t at = k * kMemcpyPiece, bytes = h.nbytes - at < kMemcpyPiece ? h.nbytes - at : kMemcpyPiece;
            blocks[ch.blk0 + k] = { (uint64_t)(uintptr_t)(in + kBloscHeader + at), (uint64_t)(uintptr_t)(dst + at), bytes, 1u, (uint32_t)kBloscCopy, i };
        }
        return;
    }
    uint64_t ga = ch.strm0, gd = ch.dstrm0;
    blosc_walk(in, len, h, [&](const BloscStream& s) {
        const bool d = direct(s.block);
        const uint64_t g = d ? gd++ : ga++;
        const uint64_t at = in_off[i] + s.src_off, to = (d ? out_off[i] : ch.slot0) + s.dst_off;     // (from the caller's base / the scratch)
        r.b.in_off[g] = at; r.b.in_len[g] = s.stored ? 0 : s.src_len;
        r.b.out_off[g] = to; r.b.out_cap[g] = s.stored ? 0 : s.dst_len;
        r.cp_src[g] = (uint64_t)(uintptr_t)(in_base + at); r.cp_dst[g] = to; r.cp_len[g] = s.stored ? s.dst_len : 0;
    }, rflags);
    uint64_t k = ch.blk0;
    for (uint32_t b = 0; b < h.nblocks; b++) {
        if (direct(b)) continue;
        const uint32_t at = b * h.blocksize, bytes = bl_block_bytes(h.nbytes, h.blocksize, b);
        blocks[k++] = { (uint64_t)(uintptr_t)(scratch + ch.slot0 + at), (uint64_t)(uintptr_t)(dst + at), bytes, h.typesize,
                        blosc_block_mode(h.flags, h.typesize, bytes), i };
    }
}

// result[i] = nbytes, the walk's error, or CJ_E_CORRUPT when a stream did not decode to exactly its length
__global__ __launch_bounds__(kBlockThreads) void bl_verdict_kernel(uint32_t n, const BlChunk* tab, CopyRows r, int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const BlChunk ch = tab[i];
    int64_t v = ch.err != 0 ? ch.err : (int64_t)ch.nbytes;
    for (uint64_t g = ch.strm0; v >= 0 && g < ch.strm0 + ch.nstr; g++)
        if (r.b.out_cap[g] != 0 && r.b.result[g] != (int64_t)r.b.out_cap[g]) v = CJ_E_CORRUPT;
    for (uint64_t g = ch.dstrm0; v >= 0 && g < ch.dstrm0 + ch.ndir; g++)
        if (r.b.out_cap[g] != 0 && r.b.result[g] != (int64_t)r.b.out_cap[g]) v = CJ_E_CORRUPT;
    result[i] = v;
}

__host__ __device__ inline uint32_t bl_filter_flags(const cj_blosc_params& p) {
    return p.filter == CJ_BLOSC_SHUFFLE ? kBloscShuffle : p.filter == CJ_BLOSC_BITSHUFFLE ? kBloscBitshuffle : 0u;
}

// compress: the filter block rows (input -> scratch) of the blocks that are transposed, and the stream rows of every chunk: streams of
// such blocks are read from the scratch, the others straight from the input (rows from the caller's base)
__global__ __launch_bounds__(kBlockThreads) void bl_pieces_kernel(uint32_t n, const BlChunk* tab, const uint8_t* in_base, const uint64_t* in_off,
                                                                  cj_blosc_params p, BatchRows b, BloscBlockRow* blocks, uint8_t* scratch) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const BlChunk ch = tab[i];
    if (ch.err != 0 || ch.nstr + ch.ndir == 0) return;
    const uint32_t flags = bl_filter_flags(p);
    const BloscLayout l = blosc_layout(ch.nbytes, p.typesize, p.blocksize);
    const uint8_t* in = in_base + in_off[i];
    uint64_t ga = ch.strm0, gd = ch.dstrm0, kb = ch.blk0, co = ch.cslot0;
    for (uint32_t k = 0; k < l.nblocks; k++) {
        const uint32_t at = k * l.blocksize, bytes = bl_block_bytes(ch.nbytes, l.blocksize, k);
        const uint32_t mode = blosc_block_mode(flags, p.typesize, bytes);
        if (mode != kBloscCopy)
            blocks[kb++] = { (uint64_t)(uintptr_t)(in + at), (uint64_t)(uintptr_t)(scratch + ch.slot0 + at), bytes, p.typesize, mode, i };
        const uint32_t ns = (l.split && bytes == l.blocksize) ? p.typesize : 1u, each = bytes / ns;
        for (uint32_t j = 0; j < ns; j++) {
            const uint64_t g = mode != kBloscCopy ? ga++ : gd++;
            b.in_off[g] = (mode != kBloscCopy ? ch.slot0 : in_off[i]) + at + j * each; b.in_len[g] = each;
            b.out_off[g] = co; b.out_cap[g] = bl_enc_room(each);
            co += bl_enc_room(each);
        }
    }
}

__device__ __forceinline__ void bl_copy64(uint8_t* dst, const uint8_t* src, uint64_t n) {
    for (uint64_t o = 0; o < n; o += (1u << 30)) wave_copy(dst + o, src + o, (uint32_t)(n - o < (1u << 30) ? n - o : (1u << 30)));
}
__device__ __forceinline__ void bl_put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// compress: one wavefront per chunk.  Sizes first (the chunk is written only when it fits, memcpyed when that is not larger), then
// header, bstarts, and stream after stream: its word and its payload — from the compressed slot, or stored from where the encoder read it
__global__ __launch_bounds__(kBlockThreads) void bl_assemble_kernel(uint32_t n, const BlChunk* tab, cj_blosc_params p, BatchRows b, const uint8_t* in_base,
                                                                    const uint64_t* in_off, const uint8_t* filtered, const uint8_t* packed,
                                                                    uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const BlChunk ch = tab[i];
    const uint32_t lane = lane_id();
    if (ch.err != 0) { if (lane == 0) result[i] = ch.err; return; }
    uint8_t* out = out_base + out_off[i];
    const uint64_t cap = out_cap[i];
    const BloscLayout l = blosc_layout(ch.nbytes, p.typesize, p.blocksize);
    const uint32_t fflags = bl_filter_flags(p);
    uint32_t flags = fflags | (l.split ? 0u : kBloscNoSplit) | (kBloscFormatLz4 << 5);
    const auto stream_bytes = [&](uint64_t g) {
        const int64_t r = b.result[g];
        return (r > 0 && (uint64_t)r < b.in_len[g]) ? (uint64_t)r : b.in_len[g];
    };
    uint64_t total = 0;
    const bool any = ch.nstr + ch.ndir != 0;
    if (any) {
        unsigned long long part = 0;
        for (uint64_t g = ch.strm0 + lane; g < ch.strm0 + ch.nstr; g += 64) part += 4 + stream_bytes(g);
        for (uint64_t g = ch.dstrm0 + lane; g < ch.dstrm0 + ch.ndir; g += 64) part += 4 + stream_bytes(g);
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        total = kBloscHeader + 4ull * l.nblocks + part;
    }
    const bool memcpyed = !any || total >= (uint64_t)ch.nbytes + kBloscHeader;
    if (memcpyed) { total = (uint64_t)ch.nbytes + kBloscHeader; flags |= kBloscMemcpyed; }
    if (total > cap) { if (lane == 0) result[i] = CJ_E_COMPRESS_FAILED; return; }
    if (lane == 0) {
        out[0] = 2; out[1] = 1; out[2] = (uint8_t)flags; out[3] = (uint8_t)p.typesize;
        bl_put32(out + 4, ch.nbytes); bl_put32(out + 8, l.blocksize); bl_put32(out + 12, (uint32_t)total);
        result[i] = (int64_t)total;
    }
    if (memcpyed) { bl_copy64(out + kBloscHeader, in_base + in_off[i], ch.nbytes); return; }
    uint64_t pos = kBloscHeader + 4ull * l.nblocks, ga = ch.strm0, gd = ch.dstrm0;
    for (uint32_t k = 0; k < l.nblocks; k++) {
        const uint32_t bytes = bl_block_bytes(ch.nbytes, l.blocksize, k);
        const bool direct = blosc_block_mode(fflags, p.typesize, bytes) == kBloscCopy;
        const uint32_t ns = (l.split && bytes == l.blocksize) ? p.typesize : 1u;
        if (lane == 0) bl_put32(out + kBloscHeader + 4 * k, (uint32_t)pos);
        for (uint32_t j = 0; j < ns; j++) {
            const uint64_t g = direct ? gd++ : ga++;
            const uint32_t each = (uint32_t)b.in_len[g], cb = (uint32_t)stream_bytes(g);
            if (lane == 0) bl_put32(out + pos, cb);
            wave_copy(out + pos + 4, cb == each ? (direct ? in_base : filtered) + b.in_off[g] : packed + b.out_off[g], cb);
            pos += 4 + cb;
        }
    }
}

// nbytes of each chunk after the header checks (cj_blosc_chunk_sizes_*): one lane per chunk
__global__ __launch_bounds__(kBlockThreads) void bl_sizes_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result,
                                                                 uint32_t rflags) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    BloscHeader h;
    const int64_t err = blosc_header(in_base + in_off[i], (size_t)in_len[i], h, rflags);
    result[i] = err != 0 ? err : (int64_t)h.nbytes;
}

}  // namespace cj

namespace {

using cj::BlChunk;
using cj::BlCount;

using cj::lane_grid;
using cj::up16;

// flags: any subset of CJ_BLOSC_FLAG_READ_BLOSCLZ / _ZLIB / _ZSTD for reading, 0 for writing (bits 0 and 2 and every higher bit stay reserved)
constexpr uint32_t kReadFlags = CJ_BLOSC_FLAG_READ_BLOSCLZ | CJ_BLOSC_FLAG_READ_ZLIB | CJ_BLOSC_FLAG_READ_ZSTD;
bool flags_ok(uint32_t flags, bool reading) { return flags == 0 || (reading && (flags & ~kReadFlags) == 0); }

int params_check(cj_op op, const cj_blosc_params* p) {
    if (op == CJ_OP_DECOMPRESS) return 0;
    if (op != CJ_OP_COMPRESS || !p || p->typesize == 0 || p->typesize > 255 || p->clevel < 0 || p->clevel > 9) return CJ_E_BAD_ARG;
    if (p->filter > CJ_BLOSC_BITSHUFFLE || (p->codec != CJ_BLOSC_LZ4 && p->codec != CJ_BLOSC_LZ4HC)) return CJ_E_BLOSC_UNSUPPORTED;
    return 0;
}

int blosc_batch(cj_engine* e, cj_op op, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, const cj_blosc_params* params, uint32_t rflags, hipStream_t s) {
    cj::ScratchTurn turn(e->fb, s);            // (the frame batches' scratch: chunk batches and frame batches on one engine run one after another)
    if (turn.rc != 0) return turn.rc;
    const bool dec = op == CJ_OP_DECOMPRESS;
    const size_t tab = up16(n * sizeof(BlChunk)), cnt_bytes = n * sizeof(BlCount);
    int rc;
    if ((rc = turn.reserve(e->d_fb, std::max(cnt_bytes, tab))) != 0 || (rc = turn.reserve(e->h_fb, tab + cnt_bytes)) != 0) return rc;
    BlChunk* h_tab = reinterpret_cast<BlChunk*>(e->h_fb.p);
    uint8_t* h_cnt = e->h_fb.p + tab;
    // the one wait: stream and block counts (decompress) / lengths (compress) size the rows, the scratch and the grids
    if (dec) {
        hipLaunchKernelGGL(cj::bl_walk_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, out_base, out_off, out_cap,
                           (BlCount*)e->d_fb.p, (const BlChunk*)nullptr, cj::CopyRows{}, (cj::BloscBlockRow*)nullptr, (uint8_t*)nullptr, rflags);
        HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
        HIP_TRY(hipMemcpyAsync(h_cnt, e->d_fb.p, cnt_bytes, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    } else {
        HIP_TRY(hipMemcpyAsync(h_cnt, in_len, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    }
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    // sa[f] / sd[f]: scratch / direct streams of the chunks of format class f (a chunk's streams are all of its one format)
    uint64_t sa[cj::kBlClasses] = {}, sd[cj::kBlClasses] = {}, nb = 0, slot = 0, cslot = 0;
    uint32_t maxlen = 0, tiles = 1;
    std::memset(h_tab, 0, n * sizeof(BlChunk));
    const auto cls = [&](size_t i) { return dec ? cj::bl_class(reinterpret_cast<const BlCount*>(h_cnt)[i].format) : 0; };
    for (size_t i = 0; i < n; i++) {
        BlChunk& c = h_tab[i];
        const int z = cls(i);
        c.strm0 = sa[z]; c.dstrm0 = sd[z]; c.blk0 = nb; c.slot0 = slot; c.cslot0 = cslot;
        if (dec) {
            const BlCount& k = reinterpret_cast<const BlCount*>(h_cnt)[i];
            c.err = k.err; c.nstr = k.nstr; c.ndir = k.ndir; c.nblk = k.nblk; c.nbytes = k.nbytes;
            if (k.scratch) slot += up16(k.nbytes);
            if (z == 0) maxlen = std::max(maxlen, k.maxlen);              // (the engine's size classes are about the LZ4 streams alone)
            tiles = std::max(tiles, k.tiles);
        } else {
            const uint64_t len = reinterpret_cast<const uint64_t*>(h_cnt)[i];
            if (len > cj::kBloscMaxBytes) { c.err = CJ_E_INPUT_TOO_LARGE; continue; }
            c.nbytes = (uint32_t)len;
            if (params->clevel == 0 || len < 32) continue;                 // memcpyed: no streams
            const cj::BloscLayout l = cj::blosc_layout(c.nbytes, params->typesize, params->blocksize);
            const uint32_t full = c.nbytes / l.blocksize, rest = c.nbytes % l.blocksize, per = l.split ? params->typesize : 1u;
            const uint32_t fl = cj::bl_filter_flags(*params);
            const bool full_f = cj::blosc_block_mode(fl, params->typesize, l.blocksize) != cj::kBloscCopy;
            const bool rest_f = rest && cj::blosc_block_mode(fl, params->typesize, rest) != cj::kBloscCopy;
            (full_f ? c.nstr : c.ndir) += full * per;
            if (rest) (rest_f ? c.nstr : c.ndir) += 1;
            c.nblk = (full_f ? full : 0u) + (rest_f ? 1u : 0u);
            if (c.nblk) { slot += up16(c.nbytes); tiles = std::max(tiles, cj::blosc_tiles(params->typesize, l.blocksize)); }
            cslot += (uint64_t)full * per * cj::bl_enc_room(l.blocksize / per) + (rest ? cj::bl_enc_room(rest) : 0);
        }
        sa[z] += c.nstr; sd[z] += c.ndir; nb += c.nblk;
    }
    // rows: scratch LZ4 | BloscLZ | Zlib | Zstd, then direct LZ4 | BloscLZ | Zlib | Zstd; a0[f] / d0[f]: where class f begins in either half
    uint64_t a0[cj::kBlClasses], d0[cj::kBlClasses], ta = 0, td = 0;
    for (int f = 0; f < cj::kBlClasses; f++) { a0[f] = ta; ta += sa[f]; }
    for (int f = 0; f < cj::kBlClasses; f++) { d0[f] = ta + td; td += sd[f]; }
    const uint64_t ns = ta + td;
    if (ns > 0xFFFFFFF0ull || nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    for (size_t i = 0; i < n; i++) { h_tab[i].strm0 += a0[cls(i)]; h_tab[i].dstrm0 += d0[cls(i)]; }
    // d_fb: chunk table | stream rows | block rows | scratch (the filtered images of chunks with transposed blocks) | compressed slots (compress)
    const size_t o_rows = tab, o_blocks = o_rows + cj::kCopyRowWords * 8 * ns, o_scr = up16(o_blocks + nb * sizeof(cj::BloscBlockRow));
    const size_t o_packed = o_scr + slot + 16;
    if ((rc = turn.reserve(e->d_fb, o_packed + cslot + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    BlChunk* d_tab = reinterpret_cast<BlChunk*>(d);
    const cj::CopyRows r = cj::copy_rows(reinterpret_cast<uint64_t*>(d + o_rows), ns);
    cj::BloscBlockRow* blocks = reinterpret_cast<cj::BloscBlockRow*>(d + o_blocks);
    uint8_t* scratch = d + o_scr;
    uint8_t* packed = d + o_packed;
    HIP_TRY(hipMemcpyAsync(d_tab, h_tab, n * sizeof(BlChunk), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    if (dec) {
        hipLaunchKernelGGL(cj::bl_walk_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, out_base, out_off, out_cap,
                           (BlCount*)nullptr, (const BlChunk*)d_tab, r, blocks, scratch, rflags);
        // format by format: streams of transposed blocks into the scratch, the others straight into the callers' slots
        for (int f = 0; f < cj::kBlClasses; f++) {
            if ((rc = cj::inner_decode(e, cj::bl_inner(f), maxlen, in_base, scratch, r.b.sub(a0[f], sa[f]), s)) != 0) return rc;
            if ((rc = cj::inner_decode(e, cj::bl_inner(f), maxlen, in_base, out_base, r.b.sub(d0[f], sd[f]), s)) != 0) return rc;
        }
        cj::launch_copy_segments(r.cp_src, scratch, r.cp_dst, r.cp_len, nullptr, 0, (uint32_t)ta, s);
        cj::launch_copy_segments(r.cp_src + ta, out_base, r.cp_dst + ta, r.cp_len + ta, nullptr, 0, (uint32_t)td, s);
        hipLaunchKernelGGL(cj::bl_verdict_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, (const BlChunk*)d_tab, r, result);
        cj::launch_blosc_filter(blocks, nb, tiles, false, result, s);
    } else {
        hipLaunchKernelGGL(cj::bl_pieces_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, (const BlChunk*)d_tab, in_base, in_off, *params, r.b, blocks, scratch);
        cj::launch_blosc_filter(blocks, nb, tiles, true, nullptr, s);
        if ((rc = cj::inner_encode(e, cj::kInLz4Raw, scratch, packed, r.b, (uint32_t)sa[0], s)) != 0) return rc;
        if ((rc = cj::inner_encode(e, cj::kInLz4Raw, in_base, packed, r.b.sub(sa[0], sd[0]), (uint32_t)sd[0], s)) != 0) return rc;
        hipLaunchKernelGGL(cj::bl_assemble_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s,
                           (uint32_t)n, (const BlChunk*)d_tab, *params, r.b, in_base, in_off, scratch, packed, out_base, out_off, out_cap, result);
    }
    return turn.done(s);
}

}  // namespace

extern "C" {

size_t cj_blosc_chunk_max_compressed_len(size_t n) { return n + 32; }

int64_t cj_blosc_chunk_info(const uint8_t* in, size_t n, cj_blosc_info* info) {
    if (!info || (n && !in)) return CJ_E_BAD_ARG;
    cj::BloscHeader h;
    const int64_t err = cj::blosc_header(in, n, h);
    *info = { h.version, h.versionlz, h.flags, h.typesize, h.nbytes, h.blocksize, h.cbytes, h.nblocks };
    return err;
}

int cj_blosc_batch_device(cj_engine* e, cj_op op, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                          const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, size_t n, const cj_blosc_params* params, uint32_t flags,
                          void* hip_stream) {
    if (!flags_ok(flags, op == CJ_OP_DECOMPRESS) || n > 0xFFFFFFF0ull || (op != CJ_OP_DECOMPRESS && op != CJ_OP_COMPRESS)) return CJ_E_BAD_ARG;
    const int pc = params_check(op, params);           // (before n == 0)
    if (pc != 0) return pc;
    return cj::device_call(e, n, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return blosc_batch(e, op, n, in_base, in_off, in_len, out_base, out_off, out_cap, result, params, flags, s);
    });
}

int cj_blosc_batch_host(cj_engine* e, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                        uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result, const cj_blosc_params* params) {
    if (!flags_ok(flags, op == CJ_OP_DECOMPRESS) || n > 0xFFFFFFF0ull || (op != CJ_OP_DECOMPRESS && op != CJ_OP_COMPRESS)) return CJ_E_BAD_ARG;
    const int pc = params_check(op, params);
    if (pc != 0) return pc;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, true,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return blosc_batch(e, op, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, params, flags, s);
    });
}

int64_t cj_blosc_chunk_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    int64_t r = 0;
    uint8_t dummy = 0;
    uint8_t* outs[1] = { out ? out : &dummy };
    const int rc = cj_blosc_batch_host(nullptr, CJ_OP_DECOMPRESS, 0, 1, &in, &n, outs, &cap, &r, nullptr);
    return rc != 0 ? rc : r;
}

int64_t cj_blosc_chunk_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, const cj_blosc_params* params) {
    int64_t r = 0;
    const int rc = cj_blosc_batch_host(nullptr, CJ_OP_COMPRESS, 0, 1, &in, &n, &out, &cap, &r, params);
    return rc != 0 ? rc : r;
}

int cj_blosc_chunk_sizes_device(cj_engine* e, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                int64_t* result, void* hip_stream) {
    if (!flags_ok(flags, true)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        hipLaunchKernelGGL(cj::bl_sizes_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, result, flags);
        HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
        return 0;
    });
}

int cj_blosc_chunk_sizes_host(cj_engine* e, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!flags_ok(flags, true) || n > 0xFFFFFFF0ull || (n && (!in_ptrs || !in_lens || !result))) return CJ_E_BAD_ARG;
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++)
        if (in_lens[i] && !in_ptrs[i]) return CJ_E_BAD_ARG;
    if (!e) e = cj::default_engine();
    if (!e) return CJ_E_NO_DEVICE;
    // (only the 16 header bytes of every chunk travel)
    std::lock_guard<std::mutex> lock(e->mu);
    HIP_TRY(hipSetDevice(e->device), CJ_E_NO_DEVICE);
    if (!e->d_in.reserve(16 * n + 16) || !e->d_meta.reserve(3 * n * 8) || !e->h_in.reserve(16 * n + 2 * n * 8)) return CJ_E_OOM;
    uint64_t* h_rows = reinterpret_cast<uint64_t*>(e->h_in.p + 16 * n);
    for (size_t i = 0; i < n; i++) {
        const size_t k = std::min<size_t>(in_lens[i], 16);
        if (k) std::memcpy(e->h_in.p + 16 * i, in_ptrs[i], k);
        // the walk checks cbytes against the bytes given: the length stays the chunk's, only the header is read
        h_rows[i] = 16 * i; h_rows[n + i] = in_lens[i];
    }
    uint64_t* d_rows = (uint64_t*)e->d_meta.p;
    HIP_TRY(hipMemcpyAsync(e->d_in.p, e->h_in.p, 16 * n, hipMemcpyHostToDevice, e->stream), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(d_rows, h_rows, 2 * n * 8, hipMemcpyHostToDevice, e->stream), CJ_E_NO_DEVICE);
    hipLaunchKernelGGL(cj::bl_sizes_kernel, lane_grid(n), dim3(cj::kBlockThreads), 0, e->stream, (uint32_t)n, (const uint8_t*)e->d_in.p, d_rows, d_rows + n,
                       (int64_t*)(d_rows + 2 * n), flags);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(result, d_rows + 2 * n, n * 8, hipMemcpyDeviceToHost, e->stream), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(e->stream), CJ_E_NO_DEVICE);
    return 0;
}

}  // extern "C"
