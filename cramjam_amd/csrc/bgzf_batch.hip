// bgzf_batch.hip — batches of BGZF streams (cj_bgzf_batch_device / _host, cj_bgzf_sizes_device / _host, cj_bgzf_compress_bound;
// DESIGN.md §5.16): the blocked gzip of BAM, BCF, tabix-indexed VCF and every `bgzip` file.  A stream is gzip members of at most
// 64 KiB that state their own length, so every member of every stream is one entry of a batch the engine already runs: the gzip
// member decoder (deflate.hip) and the DEFLATE encoder (deflate_encode.hip) are the inner kernels, unchanged.  This file is the
// container around them, in the shell of cj_container.hpp (the count pass, the one read-back, the row scan; the encoder's piece turns):
// what is BGZF's own is the hop walk (bgzf_grammar.hpp, one lane per stream, in both passes), the member rows, the stream-order verdict
// (one wavefront per stream), and for the encoder the layout (one wavefront per stream) and the assembly (one wavefront per member).
#include "cj_codecs.hpp"
#include "cj_container.hpp"
#include "bgzf_grammar.hpp"


namespace cj {

namespace {

// cj_deflate_compress_bound(n, CJ_DEFLATE_GZIP), for the arithmetic that has to hold at compile time (tests compare the two)
constexpr uint64_t gzip_bound(uint64_t n) { return n + 10u * (n / 65536u) + 5u * ((n % 65536u != 0u || n == 0u) ? 1u : 0u) + 18u; }
// a member of p input bytes at most: the encoder's stream with its 10-byte header replaced by the 18-byte one
constexpr uint64_t member_bound(uint64_t p) { return gzip_bound(p) - 10u + kBgzfHead; }
// A piece below 65 536 bytes is one DEFLATE block, at worst a stored one: the largest member is 65 311 bytes and fits BSIZE
static_assert(member_bound(kBgzfPiece) == 65311u && member_bound(kBgzfPiece) <= 65536u, "a full piece's worst case must fit BSIZE");
constexpr uint64_t kSlotStride = up16(gzip_bound(kBgzfPiece));      // a bound-sized scratch slot per member in flight

constexpr uint64_t bgzf_bound(uint64_t n) {
    return (n / kBgzfPiece) * member_bound(kBgzfPiece) + (n % kBgzfPiece ? member_bound(n % kBgzfPiece) : 0u) + kBgzfMarker;
}

}  // namespace

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
// Pass 1, and alone the size query (st == nullptr: result[i] = the ISIZE sum or the walk's error; out_cap is not read)
__global__ __launch_bounds__(kBlockThreads) void bgzf_count_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                   const uint64_t* out_cap, StreamRow* st, int64_t* result) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    uint64_t total = 0, nm = 0;
    int64_t err = bgzf_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t, uint32_t, uint32_t isize) { nm++; total += isize; });
    if (st == nullptr) { result[i] = err ? err : (int64_t)total; return; }
    if (err == 0 && total > out_cap[i]) err = CJ_E_OUT_TOO_SMALL;
    st[i] = StreamRow{0, total, err, err ? 0 : nm};
}

// Pass 2: the same walk writes one row per member — the member in the stream, its ISIZE bytes of the caller's slot behind the members
// before it.  The rows were counted from the same bytes; should they have changed since, a member the count does not cover or whose
// bytes would pass the verified sum gets no room, and a row the walk no longer reaches is an empty one.
__global__ __launch_bounds__(kBlockThreads) void bgzf_rows_kernel(uint32_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                                                  const uint64_t* out_off, const StreamRow* st, BatchRows r) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const StreamRow f = st[i];
    if (f.count == 0) return;
    uint64_t k = 0, run = 0;
    bgzf_walk(in_base + in_off[i], (size_t)in_len[i], [&](uint64_t off, uint32_t len, uint32_t isize) {
        if (k < f.count && run + isize <= f.total) {
            const uint64_t g = f.row0 + k;
            r.in_off[g] = in_off[i] + off; r.in_len[g] = len;
            r.out_off[g] = out_off[i] + run; r.out_cap[g] = isize;
            r.result[g] = 0;
            k++; run += isize;
        }
    });
    for (; k < f.count; k++) {
        const uint64_t g = f.row0 + k;
        r.in_off[g] = in_off[i]; r.in_len[g] = 0; r.out_off[g] = out_off[i]; r.out_cap[g] = 0; r.result[g] = 0;
    }
}

// One wavefront per stream: the walk's error first, then the first failing member in stream order (the lanes stride over the member
// results, a wave-wide minimum finds it).  A member's CJ_E_OUT_TOO_SMALL means that it holds more than its own ISIZE says: zlib's
// "incorrect length check".
__global__ __launch_bounds__(kBlockThreads) void bgzf_verdict_kernel(uint32_t n, const StreamRow* st, const int64_t* mres, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n) return;
    const StreamRow f = st[i];
    int64_t res = f.err ? f.err : (int64_t)f.total;
    if (f.count) {
        const unsigned long long first = first_failing_row(f.count, [&](uint64_t k) { return mres[f.row0 + k] < 0; });
        if (first != ~0ull) {
            res = mres[f.row0 + first];
            if (res == CJ_E_OUT_TOO_SMALL) res = CJ_E_DEFLATE_CHECKSUM;
        }
    }
    if (lane_id() == 0) result[i] = res;
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------------
// One row per stream.  The pieces of all streams are numbered through; they go through the encoder in turns of as many as there are
// scratch slots.  mode: 0 the capacity holds the bound — nothing can fail, members are assembled as their turn comes; 1 a smaller
// capacity, all pieces in one turn — the total is known before any store; 2 a smaller capacity across turns — the first pass only
// sizes the stream, a second pass over its turns encodes it again (the bytes depend on nothing but the input) and assembles it.
struct BgEnc {
    uint64_t piece0, pos;      // first piece; bytes of the members before the current turn
    int64_t err;               // CJ_E_INPUT_TOO_LARGE (host), a member's error
    uint32_t npiece, mode;
    uint32_t write, retry;     // this turn's members are assembled; mode 2: the stream fits, the second pass writes it
};

__device__ __forceinline__ void bgzf_put_head(uint8_t* p, uint32_t tail, uint32_t bytes) {
    // 1f 8b 08 04 | MTIME 0 | XFL 0, OS 255 | XLEN 6 | 'B' 'C' 2 0 | `tail`: BSIZE (a member) / BSIZE 27, an empty fixed block, CRC32 0, ISIZE 0
    const uint32_t l = lane_id();
    const uint64_t w = l < 8u ? 0x0000000004088b1full : l < 16u ? 0x000243420006ff00ull : (uint64_t)tail;
    if (l < bytes) p[l] = l < 24u ? (uint8_t)(w >> (8u * (l & 7u))) : (uint8_t)0;
}

// the streams without a piece: an empty buffer is the marker alone; a buffer above the limit its error
__global__ __launch_bounds__(kBlockThreads) void bgzf_empty_kernel(uint32_t n, const BgEnc* enc, uint8_t* out_base, const uint64_t* out_off,
                                                                   const uint64_t* out_cap, int64_t* result) {
    const uint32_t i = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (i >= n || enc[i].npiece != 0u) return;
    int64_t res = enc[i].err;
    if (res == 0) {
        res = out_cap[i] >= kBgzfMarker ? (int64_t)kBgzfMarker : (int64_t)CJ_E_OUT_TOO_SMALL;
        if (res > 0) bgzf_put_head(out_base + out_off[i], 0x03001bu, kBgzfMarker);
    }
    if (lane_id() == 0) result[i] = res;
}

// One wavefront per stream sa + w of a turn: the sizes of its members of this turn into their offsets in the stream, 64 at a time by
// a wave prefix sum behind what the turns before left; with the stream's last member its result — the total with the marker,
// CJ_E_OUT_TOO_SMALL when that does not fit out_cap, or a member's error.  Runs before the turn's assembly: a stream that fails
// writes nothing.
__global__ __launch_bounds__(kBlockThreads) void bgzf_layout_kernel(uint64_t t0, uint32_t cnt, uint32_t sa, uint32_t ns, uint32_t pass, BgEnc* enc,
                                                                    const int64_t* mres, uint64_t* moff, const uint64_t* out_cap, int64_t* result) {
    const uint32_t w = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (w >= ns) return;
    const uint32_t i = sa + w, lane = lane_id();
    const BgEnc f = enc[i];
    if (f.npiece == 0u) return;
    const uint64_t end = f.piece0 + f.npiece;
    const uint64_t lo = f.piece0 > t0 ? f.piece0 : t0, hi = end < t0 + cnt ? end : t0 + cnt;
    if (lo >= hi) return;
    if (pass != 0u && !(f.mode == 2u && f.retry)) {                       // the second pass is for the streams that asked for it
        if (lane == 0u) enc[i].write = 0u;
        return;
    }
    uint64_t pos = lo == f.piece0 ? 0u : f.pos;
    int64_t err = lo == f.piece0 ? 0 : f.err;
    for (uint64_t b = lo; b < hi; b += 64u) {
        const uint64_t k = b + lane;
        const bool in = k < hi;
        const int64_t v = in ? mres[k - t0] : 0;
        const uint64_t bad = ballot64(in && v < 0);
        if (bad && err == 0) err = mres[b + ctz64(bad) - t0];
        const uint32_t m = in && v >= 0 ? (uint32_t)v - 10u + kBgzfHead : 0u;
        const uint32_t inc = wave_incl_scan(m);
        if (in) moff[k - t0] = pos + (inc - m);
        pos += rdlane(inc, 63);
    }
    uint32_t write = (f.mode == 0u || pass != 0u) ? 1u : 0u, retry = f.retry;
    if (hi == end) {
        const uint64_t total = pos + kBgzfMarker;
        const int64_t r = err ? err : total <= out_cap[i] ? (int64_t)total : (int64_t)CJ_E_OUT_TOO_SMALL;
        if (f.mode == 1u) write = r >= 0 ? 1u : 0u;
        if (f.mode == 2u && pass == 0u) retry = r >= 0 ? 1u : 0u;
        if (lane == 0u && !(f.mode == 2u && pass == 0u && r >= 0)) result[i] = r;
    }
    if (lane == 0u) { enc[i].pos = pos; enc[i].err = err; enc[i].write = write; enc[i].retry = retry; }
}

// One wavefront per member of a turn: the 18-byte header, then the slot from byte 10 on (the DEFLATE data, CRC32 and ISIZE); the last
// member's wavefront writes the marker behind it.
__global__ __launch_bounds__(kBlockThreads) void bgzf_assemble_kernel(uint64_t t0, uint32_t cnt, const BgEnc* enc, const uint32_t* owner, const int64_t* mres,
                                                                      const uint64_t* moff, const uint8_t* slots, uint64_t stride, uint8_t* out_base,
                                                                      const uint64_t* out_off) {
    const uint32_t j = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (j >= cnt) return;
    const uint32_t i = uni(owner[j]);
    const int64_t c = mres[j];
    if (enc[i].write == 0u || c < 20 || (uint64_t)c > stride) return;     // (a slot holds a header, a block and the trailer)
    uint8_t* dst = out_base + out_off[i] + moff[j];
    const uint32_t body = (uint32_t)c - 10u;
    bgzf_put_head(dst, body + kBgzfHead - 1u, kBgzfHead);
    wave_copy(dst + kBgzfHead, slots + (uint64_t)j * stride + 10u, body);
    if (t0 + j + 1u == enc[i].piece0 + enc[i].npiece) bgzf_put_head(dst + kBgzfHead + body, 0x03001bu, kBgzfMarker);
}

}  // namespace cj

namespace {

using cj::BgEnc;

// bytes of bound-sized member slots per turn of a compress batch at most: 4096 slots
cj::SlotBudget g_slot_budget{4096ull * cj::kSlotStride};

// enqueue only: pass 1 with the results straight into the caller's row
int bgzf_sizes(size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, int64_t* result, hipStream_t s) {
    hipLaunchKernelGGL(cj::bgzf_count_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, nullptr, nullptr, result);
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    return 0;
}

int bgzf_decode(cj_engine* e, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off,
                const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch, held across the call's one wait (cj_container.hpp)
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    cj::StreamTable t;
    int rc = cj::stream_table(turn, e, n, cj::kBatchRowWords, s, [&](cj::StreamRow* d_st) {
        hipLaunchKernelGGL(cj::bgzf_count_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, out_cap, d_st, nullptr);
    }, t);
    if (rc != 0) return rc;
    const cj::StreamRow* st = t.st;
    const cj::BatchRows r = cj::batch_rows(t.rows, t.nb);
    if (t.nb) {
        hipLaunchKernelGGL(cj::bgzf_rows_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, in_base, in_off, in_len, out_off, st, r);
        if ((rc = cj::inner_decode(e, cj::kInGzip, 0, in_base, out_base, r, s)) != 0) return rc;
    }
    hipLaunchKernelGGL(cj::bgzf_verdict_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, st, r.result, result);
    return turn.done(s);
}

int bgzf_encode(cj_engine* e, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off,
                const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // The same scratch and the same one wait, for the buffers' lengths and capacities
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    bool second = false;
    cj::EncPlan<BgEnc> p;
    int rc = cj::enc_plan(turn, e, n, in_len, out_cap, cj::kSlotStride, g_slot_budget, 0, s, [&](BgEnc& x, uint64_t len, uint64_t cap, uint64_t per) {
        if (len > 0x7E000000ull) x.err = CJ_E_INPUT_TOO_LARGE;
        else x.npiece = (uint32_t)((len + cj::kBgzfPiece - 1) / cj::kBgzfPiece);
        if (x.npiece && cap < cj::bgzf_bound(len)) x.mode = x.piece0 / per == (x.piece0 + x.npiece - 1) / per ? 1u : 2u;
        second = second || x.mode == 2u;
    }, p);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(cj::bgzf_empty_kernel, cj::wave_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, p.enc, out_base, out_off, out_cap, result);
    // the second pass skips the turns that hold no mode-2 stream
    for (uint32_t pass = 0; pass < (second ? 2u : 1u); pass++) {
        const auto skip = [&](const BgEnc* a, const BgEnc* b) { return pass != 0 && std::none_of(a, b, [](const BgEnc& x) { return x.mode == 2u; }); };
        rc = cj::for_turns(p, in_off, in_len, cj::kBgzfPiece, s, skip, [&](uint64_t t0, uint32_t cnt, uint32_t sa, uint32_t ns) {
            const int erc = cj::inner_encode(e, cj::kInGzip, in_base, p.slots, p.r, cnt, s);
            if (erc != 0) return erc;
            hipLaunchKernelGGL(cj::bgzf_layout_kernel, cj::wave_grid(ns), dim3(cj::kBlockThreads), 0, s, t0, cnt, sa, ns, pass, p.enc, p.r.result, p.moff, out_cap, result);
            hipLaunchKernelGGL(cj::bgzf_assemble_kernel, cj::wave_grid(cnt), dim3(cj::kBlockThreads), 0, s, t0, cnt, p.enc, p.owner, p.r.result, p.moff, p.slots,
                               (uint64_t)cj::kSlotStride, out_base, out_off);
            return 0;
        });
        if (rc != 0) return rc;
    }
    return turn.done(s);
}

bool bgzf_args_ok(int what, cj_op op, uint32_t flags) { return what == 0 && flags == 0u && (op == CJ_OP_DECOMPRESS || op == CJ_OP_COMPRESS); }

}  // namespace

extern "C" {

size_t cj_bgzf_compress_bound(size_t n) { return n > 0x7E000000ull ? 0 : (size_t)cj::bgzf_bound(n); }

int cj_bgzf_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_streams, const uint8_t* in_base, const uint64_t* in_off,
                         const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!bgzf_args_ok(what, op, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_streams, {in_base, in_off, in_len, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        return (op == CJ_OP_DECOMPRESS ? bgzf_decode : bgzf_encode)(e, n_streams, in_base, in_off, in_len, out_base, out_off, out_cap, result, s);
    });
}

int cj_bgzf_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens,
                       uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!bgzf_args_ok(what, op, flags)) return CJ_E_BAD_ARG;
    return cj::host_call(e, n, in_ptrs, in_lens, out_ptrs, out_caps, result, -1, false,
                         [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        return (op == CJ_OP_DECOMPRESS ? bgzf_decode : bgzf_encode)(e, n, d_in, d.in_off, d.in_len, d_out, d.out_off, d.out_cap, d.result, s);
    });
}

int cj_bgzf_sizes_device(cj_engine* e, int what, uint32_t flags, size_t n_streams, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                         int64_t* result, void* hip_stream) {
    if (what != 0 || flags != 0u) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_streams, {in_base, in_off, in_len, result}, hip_stream, [&](cj_engine*, hipStream_t s) {
        return bgzf_sizes(n_streams, in_base, in_off, in_len, result, s);
    });
}

int cj_bgzf_sizes_host(cj_engine* e, int what, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result) {
    if (what != 0 || flags != 0u) return CJ_E_BAD_ARG;
    return cj::host_sizes_call(e, n, in_ptrs, in_lens, result, [&](cj_engine*, const uint8_t* d_in, const cj::BatchRows& d, hipStream_t s) {
        return bgzf_sizes(n, d_in, d.in_off, d.in_len, d.result, s);
    });
}

// tests: the bytes of member slots per turn of a BGZF compress batch (0 = the default); returns the previous value
uint64_t cj_debug_bgzf_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
