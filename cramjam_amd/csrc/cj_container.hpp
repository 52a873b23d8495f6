// cj_container.hpp — the shell of the container batches whose streams hold many entries each (bgzf_batch.hip, orc_batch.hip, parquet_batch.hip; DESIGN.md
// §5.16a): a stream's members / chunks are entries of a batch the engine already runs, so both directions are the same protocol around
// the format's own kernels.  Decode: a count pass (one lane per stream), ONE read-back and wait, the host's scan of the counts into row0,
// the rows pass, the codec, a stream-order verdict.  Encode: one read-back and wait for the buffers' lengths and capacities, the pieces
// of all streams numbered through, and turns of as many pieces as there are bound-sized scratch slots.  Not part of the C ABI.
#pragma once
#include "cj_stage.hpp"

namespace cj {

// ---- device ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane_id() >= (uint32_t)d) v += t;
    }
    return v;
}

// The first failing row in stream order, for a whole wavefront: the smallest k < count with bad(k), or ~0ull.  The lanes stride over
// the rows, each up to its own first hit; a wave-wide minimum finds the stream's.
template <class Bad>
__device__ __forceinline__ unsigned long long first_failing_row(uint64_t count, Bad&& bad) {
    unsigned long long first = ~0ull;
    for (uint64_t k = lane_id(); k < count; k += 64u)
        if (bad(k)) { first = k; break; }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const unsigned long long o = __shfl_xor(first, sh, 64);
        first = o < first ? o : first;
    }
    return first;
}

// Decode: one row per stream.  The count kernel writes total, err and count; row0 is the host's scan of the counts.
struct StreamRow {
    uint64_t row0, total;      // first entry row; the decoded length — BGZF: the ISIZE sum, Parquet: the pages' stated sizes' sum, from the count kernel; ORC: 0 until the layout kernel sums the chunks' sizes
    int64_t err;               // the walk's error; then BGZF (count kernel): CJ_E_OUT_TOO_SMALL when the ISIZE sum exceeds out_cap; ORC (layout kernel):
                               // a chunk's size error, CJ_E_ORC_BLOCK, CJ_E_OUT_TOO_SMALL
    uint64_t count;            // members / chunks the walk accepts; 0 with an error of the count kernel: such a stream has no rows
};

// Encode: the rows of pieces [t0, t0 + cnt), `piece` input bytes each (a stream's last one what is left).  Enc: the format's row per
// stream, which begins {piece0, pos, err, npiece}.  Slot j of the scratch is piece t0 + j's, owner[j] its stream (the last one that
// begins at or before the piece: streams without pieces share their successor's piece0 and lie before it)
template <class Enc>
__global__ __launch_bounds__(kBlockThreads) void piece_rows_kernel(uint64_t t0, uint32_t cnt, uint32_t n, const Enc* enc, const uint64_t* in_off,
                                                                   const uint64_t* in_len, BatchRows r, uint32_t* owner, uint64_t stride, uint32_t piece) {
    const uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x;
    if (j >= cnt) return;
    const uint64_t g = t0 + j;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (enc[mid].piece0 <= g) lo = mid + 1u; else hi = mid;
    }
    const uint32_t i = lo - 1u;                                           // (enc[0].piece0 = 0 <= g)
    const uint64_t at = (g - enc[i].piece0) * piece, len = in_len[i];
    r.in_off[j] = in_off[i] + at;
    r.in_len[j] = len - at < piece ? len - at : piece;
    r.out_off[j] = (uint64_t)j * stride;
    r.out_cap[j] = stride;
    owner[j] = i;
}

// ---- host: decode ------------------------------------------------------------------------------------------------------------------------
// What a decode has in e->d_fb behind the prologue: streams | entry rows (`words` u64 rows of nb entries each)
struct StreamTable {
    StreamRow* st;
    uint64_t* rows;
    size_t nb;
};

// The prologue, inside the caller's turn at e->fb: count(d_st) launches the format's count kernel into the device table; then the
// read-back and the call's ONE wait, the scan of the counts into row0, room for the entry rows, and the table's upload.  0 or CJ_E_*.
// seen(row) gets every stream's row as the count kernel left it, before the scan sets its row0: until then that word is the format's
// (Parquet: the largest decoded page).
template <class Count, class Seen>
int stream_table(ScratchTurn& turn, cj_engine* e, size_t n, size_t words, hipStream_t s, Count&& count, StreamTable& t, Seen&& seen) {
    const size_t tab = up16(n * sizeof(StreamRow));
    int rc;
    if ((rc = turn.reserve(e->d_fb, tab)) != 0 || (rc = turn.reserve(e->h_fb, tab)) != 0) return rc;
    StreamRow* h_st = reinterpret_cast<StreamRow*>(e->h_fb.p);
    count(reinterpret_cast<StreamRow*>(e->d_fb.p));
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(h_st, e->d_fb.p, n * sizeof(StreamRow), hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);       // the one wait: the host sizes the entry rows from the streams' counts
    uint64_t nb = 0;
    for (size_t i = 0; i < n; i++) { seen(h_st[i]); h_st[i].row0 = nb; nb += h_st[i].count; }
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    // No data scratch: the entries decode straight into the callers' slots
    if ((rc = turn.reserve(e->d_fb, tab + words * 8 * (size_t)nb + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    t = {reinterpret_cast<StreamRow*>(d), reinterpret_cast<uint64_t*>(d + tab), (size_t)nb};
    HIP_TRY(hipMemcpyAsync(t.st, h_st, n * sizeof(StreamRow), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    return 0;
}
template <class Count>
int stream_table(ScratchTurn& turn, cj_engine* e, size_t n, size_t words, hipStream_t s, Count&& count, StreamTable& t) {
    return stream_table(turn, e, n, words, s, count, t, [](const StreamRow&) {});
}

// ---- host: encode ------------------------------------------------------------------------------------------------------------------------
// What an encode has behind its plan.  e->d_fb: streams | piece rows | offsets | owners | the format's u32 per piece | slots, of `per`
// pieces at most; e->h_fb: in_len | out_cap | streams.
template <class Enc>
struct EncPlan {
    size_t n;
    uint64_t nb, per, stride;  // pieces of the batch; pieces per turn; bytes of a slot
    const Enc* h_enc;
    Enc* enc;
    BatchRows r;
    uint64_t* moff;
    uint32_t *owner, *extra;
    uint8_t* slots;
};

// The plan, inside the caller's turn at e->fb: the read-back of the lengths and capacities and the call's ONE wait; fill(x, len, cap,
// per) sets the format's fields of a stream whose piece0 is set — npiece, or err and no piece —; the limit; the layout, with `extra`
// u32 words per piece of the format's own; the table's upload.  0 or CJ_E_*.
template <class Enc, class Fill>
int enc_plan(ScratchTurn& turn, cj_engine* e, size_t n, const uint64_t* in_len, const uint64_t* out_cap, uint64_t stride, const SlotBudget& budget,
             size_t extra, hipStream_t s, Fill&& fill, EncPlan<Enc>& p) {
    const size_t tab = up16(n * sizeof(Enc));
    int rc;
    if ((rc = turn.reserve(e->h_fb, 16 * n + tab)) != 0) return rc;
    const uint64_t* h_len = reinterpret_cast<const uint64_t*>(e->h_fb.p);
    const uint64_t* h_cap = h_len + n;
    Enc* h_enc = reinterpret_cast<Enc*>(e->h_fb.p + 16 * n);
    HIP_TRY(hipMemcpyAsync((void*)h_len, in_len, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync((void*)h_cap, out_cap, 8 * n, hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);
    const uint64_t per = std::max<uint64_t>(1, budget.load() / stride);
    uint64_t nb = 0;
    for (size_t i = 0; i < n; i++) {
        Enc x = {};
        x.piece0 = nb;
        fill(x, h_len[i], h_cap[i], per);
        nb += x.npiece;
        h_enc[i] = x;
    }
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    const size_t m = (size_t)std::min(nb, per);
    const size_t o_rows = tab, o_moff = o_rows + 5 * 8 * m, o_own = o_moff + 8 * m, o_extra = o_own + 4 * m, o_slots = up16(o_extra + 4 * m * extra);
    if ((rc = turn.reserve(e->d_fb, o_slots + m * (size_t)stride + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    p = {n, nb, per, stride, h_enc, reinterpret_cast<Enc*>(d), batch_rows(reinterpret_cast<uint64_t*>(d + o_rows), m), reinterpret_cast<uint64_t*>(d + o_moff),
         reinterpret_cast<uint32_t*>(d + o_own), reinterpret_cast<uint32_t*>(d + o_extra), d + o_slots};
    HIP_TRY(hipMemcpyAsync(p.enc, h_enc, n * sizeof(Enc), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    return 0;
}

// The turns of a plan: for each the piece rows, then body(t0, cnt, sa, ns) — pieces [t0, t0 + cnt) lie in streams [sa, sa + ns).
// skip(first, last) on the host rows of those streams leaves a turn out.  0 or the body's CJ_E_*.
template <class Enc, class Skip, class Body>
int for_turns(const EncPlan<Enc>& p, const uint64_t* in_off, const uint64_t* in_len, uint32_t piece, hipStream_t s, Skip&& skip, Body&& body) {
    // the stream of piece g, as piece_rows_kernel finds it
    const auto stream_of = [&](uint64_t g) {
        return (size_t)(std::upper_bound(p.h_enc, p.h_enc + p.n, g, [](uint64_t v, const Enc& x) { return v < x.piece0; }) - p.h_enc) - 1;
    };
    for (uint64_t t0 = 0; t0 < p.nb; t0 += p.per) {
        const uint32_t cnt = (uint32_t)std::min(p.per, p.nb - t0);
        const size_t sa = stream_of(t0), sb = stream_of(t0 + cnt - 1);
        if (skip(p.h_enc + sa, p.h_enc + sb + 1)) continue;
        hipLaunchKernelGGL(piece_rows_kernel<Enc>, lane_grid(cnt), dim3(kBlockThreads), 0, s, t0, cnt, (uint32_t)p.n, p.enc, in_off, in_len, p.r, p.owner, p.stride, piece);
        const int rc = body(t0, cnt, (uint32_t)sa, (uint32_t)(sb - sa + 1));
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace cj
