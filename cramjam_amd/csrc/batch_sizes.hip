// batch_sizes.hip — decoded-size queries for batches (cj_batch_sizes_device / _host, cj_frame_batch_sizes_device / _host): what a
// caller needs to lay out out_off / out_cap BEFORE it can submit a decode, for chunks that may live in HBM only.
//   Snappy raw, prefixed LZ4   the header of each chunk, one lane per chunk
//   LZ4 frames, Snappy framed  the grammar walk of frame_grammar.hpp with a summing visitor, one lane per stream
//   LZ4 raw blocks             the size WALK (lz4_size_walk.hpp): the token chain of every chunk to its end.  One lane per chunk
//                              through the parse kernel's LDS line rings (lane_stream.hpp) for chunks of up to kSizeLaneMaxIn
//                              bytes; one wavefront per chunk through the 512-byte register window for longer ones.
// The device calls only enqueue: no wait, no read-back, no engine scratch, no lock — they may sit in front of a decode on the same
// stream, or run next to a frame batch that holds the engine's frame scratch.
#include "cj_stage.hpp"
#include "cj_codecs.hpp"
#include "frame_grammar.hpp"
#include "lane_stream.hpp"
#include "lz4_size_walk.hpp"

namespace cj {

// Chunks above this many input bytes leave the lane kernel: a lane walks ~0.55 µs per sequence whatever its neighbours do, so one
// 256 KiB chunk among 64 KiB ones would hold its wavefront (and the kernel) four times as long; a wavefront of its own walks the
// same chain ~8x quicker.  LZ4_compressBound(65536) rounded up to 16: every chunk of at most 64 KiB of data stays on a lane.
#ifndef CJ_SIZE_LANE_MAX_IN
#define CJ_SIZE_LANE_MAX_IN 65824u
#endif
constexpr uint32_t kSizeLaneMaxIn = CJ_SIZE_LANE_MAX_IN;
#ifndef CJ_SIZE_AHEAD
#define CJ_SIZE_AHEAD 32u                      // cached bytes a lane wants ahead of its position (lz4_parse_kernel's measured value)
#endif
#ifndef CJ_SIZE_EXTRA
#define CJ_SIZE_EXTRA 7                        // further straight-line sequences per trip (lz4_parse_kernel's measured value)
#endif

// ---- LZ4 raw blocks, one lane per chunk -------------------------------------------------------------------------------------------
// lz4_parse_kernel's walk (lz4_decode_lanes.hip) without a capacity: no output margins to test, no sync points, no ParseMeta, no
// routing.  The straight-line trip commits a sequence whose length fields take at most one extension byte, whose fields lie in
// the cached window at least 8 bytes before the block's end and whose match lies inside the output so far; everything else — and
// every verdict — is lz4_size_seq / lz4_size_commit from the same state.  in_len <= kSizeLaneMaxIn keeps the size below 2^25:
// the straight-line position is 32 bits wide.
__global__ __launch_bounds__(64 * kParseWaves) void lz4_size_lanes_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                          const uint64_t* in_len, int64_t* result) {
    __shared__ __attribute__((aligned(16))) uint8_t rings[kParseWaves * 64 * kRingStride];
    const uint32_t c = blockIdx.x * (64u * kParseWaves) + threadIdx.x;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t wave_ring = (uint32_t)(uintptr_t)rings + wave * 64u * kRingStride;

    const uint8_t* in = nullptr;
    uint64_t n64 = 0;
    int64_t r = 0;
    bool done = true, mine = false;
    if (c < n) {
        in = in_base + in_off[c];
        n64 = in_len[c];
        mine = true;
        if (n64 == 0 || n64 > kLz4InMax) r = CJ_E_CORRUPT;
        else if (n64 > kSizeLaneMaxIn) mine = false;               // lz4_size_wave_kernel's
        else done = false;
    }
    LaneStream st;
    const uint32_t mis = done ? 0u : (uint32_t)(reinterpret_cast<uintptr_t>(in) & 127u);
    st.base = done ? (CJ_REFILL_TOUCH ? in_base : nullptr) : in - mis;
    st.lo = 0; st.hi = 0;
#if CJ_REFILL_TOUCH
    st.touch = 0;
#endif
    st.end = done ? 0u : mis + (uint32_t)n64;
    st.ring = wave_ring + lane * kRingStride;
    const uint32_t iend = st.end;
    const RefillPlan plan = refill_plan(st);

    uint32_t ip = mis, op = 0;
    while (ballot64(!done) != 0ull) {
        if (!done && ip >= st.hi) st.lo = st.hi = ip & ~127u;      // jumped past the window (long literal run): re-anchor
        for (;;) {                                                 // refill rounds: when some lane is about to run dry, every lane with room is topped up
            const bool want = !done && st.hi < iend && (st.hi - st.lo < kRingBytes || ip >= st.lo + 128u);
            const bool urgent = want && ip + CJ_SIZE_AHEAD > st.hi;
            if (ballot64(urgent) == 0ull) break;
            refill_round(st, want, wave_ring, plan);
        }
        struct FastSeq { bool ok; uint32_t ip3, op3, t4n; };
        const uint32_t win_end = st.hi < iend ? st.hi : iend;
        const int32_t ip2_max = (int32_t)win_end - 4 < (int32_t)iend - 8 ? (int32_t)win_end - 4 : (int32_t)iend - 8;      // (signed: a short block makes it negative)
        const bool ip_low_ok = ip >= st.lo;
        // one dependent LDS round trip per sequence: the offset field and the NEXT token are read together (where that token sits
        // follows from this token alone: the extension bytes that would move it are the ones this path refuses)
        const auto fast_seq = [&](uint32_t t4) __attribute__((always_inline)) -> FastSeq {
            const uint32_t token = t4 & 0xffu, e1 = (t4 >> 8) & 0xffu;
            const bool x1 = (token >> 4) == 15u;
            const uint32_t lit = (token >> 4) + (x1 ? e1 : 0u);
            const uint32_t ip2 = ip + (x1 ? 2u : 1u) + lit;
            const uint32_t mc = token & 15u;
            const bool x2 = mc == 15u;
            const uint32_t ip3 = ip2 + (x2 ? 3u : 2u);
            const LaneStream::Pair rq = st.ring32x2_request(ip2, ip3);
            const uint32_t op2 = op + lit;
            const bool ok_early = ip_low_ok & ((int32_t)(ip + 4u) <= (int32_t)win_end) & ((int32_t)ip2 <= ip2_max) & !(x1 & (e1 == 255u));
            uint32_t o4, t4n;
            st.ring32x2_arrive(rq, ip2, ip3, o4, t4n);
            const uint32_t offset = o4 & 0xffffu, e2 = (o4 >> 16) & 0xffu;
            const uint32_t op3 = op2 + mc + (x2 ? e2 : 0u) + 4u;
            const bool ok = ok_early & !(x2 & (e2 == 255u)) & (offset != 0u) & (offset <= op2);
            return FastSeq{ok, ip3, op3, t4n};
        };
        bool fast_ok = false;
        uint32_t t4_next = 0;
        if (!done) {
            const FastSeq f = fast_seq(st.ring32(ip));
            fast_ok = f.ok; t4_next = f.t4n;
            if (f.ok) { ip = f.ip3; op = f.op3; }
        }
        bool more = fast_ok;
#pragma unroll
        for (int rep = 0; rep < CJ_SIZE_EXTRA; rep++) {
            if (ballot64(more) == 0ull) break;
            if (more) {
                const FastSeq f = fast_seq(t4_next);
                if (f.ok) { ip = f.ip3; op = f.op3; }
                more = f.ok; t4_next = f.t4n;
            }
        }
        if (!done && !fast_ok) {
            SizeSeq s;
            uint64_t op64 = op;
            const bool ok = lz4_size_seq([&](uint32_t p) { return st.ld32(p); },
                                         [&](uint32_t p, uint32_t e) { return lz4_ff_run(st.base, p, e); }, ip, iend, s)
                            && lz4_size_commit(s, op64);
            if (!ok) { r = CJ_E_CORRUPT; done = true; }
            else if (s.last) { r = lz4_size_verdict(op64); done = true; }
            else { ip = s.next; op = (uint32_t)op64; }
        }
    }
    if (mine) result[c] = r;
}

// ---- LZ4 raw blocks above kSizeLaneMaxIn bytes, one wavefront per chunk ---------------------------------------------------------------
// The position is wave-uniform; the stream is read through the 512-byte register window of the wave-per-chunk decoder (InWindow:
// any 4 bytes by v_readlane, a dependent global load only every 256 bytes), runs of length bytes straight from memory.
__global__ __launch_bounds__(kBlockThreads) void lz4_size_wave_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                      const uint64_t* in_len, int64_t* result) {
    const uint32_t c = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (c >= n) return;
    const uint64_t n64 = in_len[c];
    if (n64 <= kSizeLaneMaxIn || n64 > kLz4InMax) return;          // the lane kernel answers those
    const uint8_t* in = in_base + in_off[c];
    InWindow w;
    const uint32_t mis = window_open(w, in, (uint32_t)n64);
    const int64_t r = lz4_size_walk([&](uint32_t p) { p = uni(p); w.ensure(p); return w.fetch32(p); },
                                    [&](uint32_t p, uint32_t e) { return uni(lz4_ff_run(w.base, uni(p), e)); }, mis, w.iend);
    if (lane_id() == 0) result[c] = r;
}

// ---- headers: Snappy raw (the varint preamble), prefixed LZ4 (the u32 prefix by lz4_block_prologue's rules) ---------------------------
// Only bytes of the chunk itself are read, a chunk shorter than the field is answered from its length.
__global__ __launch_bounds__(kBlockThreads) void header_sizes_kernel(int codec, uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                     const uint64_t* in_len, int64_t* result) {
    const uint32_t c = blockIdx.x * kBlockThreads + threadIdx.x;
    if (c >= n) return;
    const uint8_t* in = in_base + in_off[c];
    uint64_t n64 = in_len[c];
    if (codec == CJ_CODEC_SNAPPY_RAW) { result[c] = snappy_varint_len(in, (size_t)n64); return; }
    uint64_t cap64 = ~0ull;                                        // (no capacity: CJ_E_OUT_TOO_SMALL cannot occur)
    const int64_t st = lz4_block_prologue(CJ_FLAG_LZ4_SIZE_PREFIX, in, n64, cap64);
    result[c] = st != 0 ? st : (int64_t)cap64;
}

// ---- framed streams: one lane per stream --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads) void frame_sizes_kernel(int fmt, uint32_t n, const uint8_t* in_base, const uint64_t* in_off,
                                                                    const uint64_t* in_len, int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t* in = in_base + in_off[i];
    const size_t len = (size_t)in_len[i];
    result[i] = fmt == CJ_FORMAT_LZ4_FRAME ? lz4_frame_bound(in, len) : snappy_frame_len(in, len);
}

}  // namespace cj

namespace {

enum class Query { Blocks, Frames };

bool known(Query q, int what) {
    return q == Query::Blocks ? (what == CJ_CODEC_LZ4_BLOCK || what == CJ_CODEC_SNAPPY_RAW) : (what == CJ_FORMAT_LZ4_FRAME || what == CJ_FORMAT_SNAPPY_FRAMED);
}
bool flags_ok(Query q, uint32_t flags) { return (flags & ~(q == Query::Blocks ? CJ_FLAG_LZ4_SIZE_PREFIX : 0u)) == 0u; }

// enqueue only
int sizes_launch(Query q, int what, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                 int64_t* result, hipStream_t s) {
    const uint32_t n32 = (uint32_t)n;
    const dim3 per_lane((n32 + cj::kBlockThreads - 1) / cj::kBlockThreads), block(cj::kBlockThreads);
    if (q == Query::Frames) {
        hipLaunchKernelGGL(cj::frame_sizes_kernel, per_lane, block, 0, s, what, n32, in_base, in_off, in_len, result);
    } else if (what == CJ_CODEC_SNAPPY_RAW || (flags & CJ_FLAG_LZ4_SIZE_PREFIX)) {
        hipLaunchKernelGGL(cj::header_sizes_kernel, per_lane, block, 0, s, what, n32, in_base, in_off, in_len, result);
    } else {
        const uint32_t per_block = 64u * cj::kParseWaves;
        hipLaunchKernelGGL(cj::lz4_size_lanes_kernel, dim3((n32 + per_block - 1u) / per_block), dim3(per_block), 0, s, n32, in_base, in_off, in_len, result);
        hipLaunchKernelGGL(cj::lz4_size_wave_kernel, cj::wave_grid(n32), block, 0, s, n32, in_base, in_off, in_len, result);
    }
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

int sizes_device(Query q, cj_engine* e, int what, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off,
                 const uint64_t* in_len, int64_t* result, void* hip_stream) {
    if (!known(q, what) || !flags_ok(q, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return sizes_launch(q, what, flags, n, in_base, in_off, in_len, result, s);
    });
}

int sizes_host(Query q, cj_engine* e, int what, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (!known(q, what) || !flags_ok(q, flags)) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return sizes_launch(q, what, flags, n, d_in, d.in_off, d.in_len, d.result, s);
    });
}

}  // namespace

int cj::launch_block_sizes(int codec, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s) {
    if (n == 0) return 0;
    return sizes_launch(Query::Blocks, codec, 0u, n, in_base, in_off, in_len, result, s);
}

extern "C" {

int cj_batch_sizes_device(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                          const uint64_t* in_len, int64_t* result, void* hip_stream) {
    return sizes_device(Query::Blocks, e, (int)codec, flags, n_chunks, in_base, in_off, in_len, result, hip_stream);
}

int cj_batch_sizes_host(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks, const uint8_t* const* in_ptrs, const size_t* in_lens,
                        int64_t* result) {
    return sizes_host(Query::Blocks, e, (int)codec, flags, n_chunks, in_ptrs, in_lens, result);
}

int cj_frame_batch_sizes_device(cj_engine* e, cj_format fmt, uint32_t flags, size_t n_frames, const uint8_t* in_base, const uint64_t* in_off,
                                const uint64_t* in_len, int64_t* result, void* hip_stream) {
    return sizes_device(Query::Frames, e, (int)fmt, flags, n_frames, in_base, in_off, in_len, result, hip_stream);
}

int cj_frame_batch_sizes_host(cj_engine* e, cj_format fmt, uint32_t flags, size_t n_frames, const uint8_t* const* in_ptrs, const size_t* in_lens,
                              int64_t* result) {
    return sizes_host(Query::Frames, e, (int)fmt, flags, n_frames, in_ptrs, in_lens, result);
}

}  // extern "C"
