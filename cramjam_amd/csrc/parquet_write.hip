// parquet_write.hip — batches of decoded Parquet column chunks INTO column chunks (cj_parquet_compress_device / _host,
// cj_parquet_compress_bound): the writer beside parquet_batch.hip's reader.  The caller gives the decoded chunk — what
// cj_parquet_batch_* writes — and its page table in the pages query's layout; every values section is one entry of a batch the engine
// already runs (Snappy raw and raw LZ4 blocks through cj::launch, gzip members, Zstandard frames: the plain encoders, unchanged), and
// this file is the container around them, on cj_container.hpp's ground (the fb turn, the one read-back, wave_incl_scan).  Pages have
// neither one size nor one slot stride, so enc_plan / for_turns do not fit; Parquet's own instead: the plan (one lane per chunk: the
// table's rules, the pages the codec sees, their 16-byte-rounded bound-sized slots), turns of WHOLE chunks under a slot budget, the
// rows (one lane per chunk), per page the choice between the codec's output and the raw values and the CRC-32 over a payload that lies
// in two places (one wavefront per page), the layout (one wavefront per chunk: header lengths from sizes and CRCs only the device
// knows, the capacity check before any store) and the assembly (one wavefront per page).
// NOT enqueue-only: a call takes one turn at the engine's container scratch and waits for the stream once, for the chunks' plans.
#include "cj_codecs.hpp"
#include "cj_container.hpp"
#include "crc32_lanes.hpp"
#include "parquet_write.hpp"

#include <vector>

namespace cj {

namespace {
__device__ const Crc32Tables d_pqw_crc32_tables = make_crc32_tables();
}

// One row per chunk.  The plan kernel leaves err, npages, ncoded and slots, the chunk's slot bytes; the host's scan sets page0, code0
// and slot0 (the offset of the chunk's slots in its turn's).  A chunk with a code of the plan has no pages.
struct PqwChunk {
    uint64_t page0, code0, slot0;
    int64_t err;
    uint64_t npages, ncoded, slots;
};

// The per-page rows, numbered through the batch, and the encoder's rows, numbered through the pages the codec sees
struct PqwRows {
    uint64_t *src, *code, *owner;           // offset of the page's decoded bytes in in_base; its encoder row or kPqwNone; its chunk
    int64_t* snap;                          // the page's table row as the rows kernel read it, eight words: what every later kernel goes by
    int64_t* pay;                           // the choice: compressed_page_size | is-codec-output << 32, or the encoder's code (V1, dictionary)
    uint64_t *crc, *out;                    // the payload's CRC-32; the layout: offset of the header in the chunk's slot, kPqwNone: not written
    BatchRows b;                            // in_base = the decoded chunks, out_base = the turn's slots
};
constexpr size_t kPqwRowWords = 6 + kPqPageWords;
constexpr uint64_t kPqwNone = ~0ull, kPqwCoded = 1ull << 32;
inline PqwRows pqw_rows(uint64_t* base, size_t nb, size_t nc) {
    PqwRows r;
    r.src = base; r.code = base + nb; r.owner = base + 2 * nb; r.pay = reinterpret_cast<int64_t*>(base + 3 * nb);
    r.crc = base + 4 * nb; r.out = base + 5 * nb; r.snap = reinterpret_cast<int64_t*>(base + 6 * nb);
    r.b = batch_rows(base + kPqwRowWords * nb, nc);
    return r;
}

// where chunk i's table lies and how many rows it has (the device call: 64-byte rows counted; the host call: staged bytes)
struct PqwTables {
    const uint8_t* tab;
    const uint64_t *off, *cnt;
    uint32_t off_unit, cnt_div;
    __device__ const int64_t* rows(uint32_t i) const { return reinterpret_cast<const int64_t*>(tab + (uint64_t)off_unit * off[i]); }
    __device__ uint64_t count(uint32_t i) const { return cnt[i] / cnt_div; }
};

// the values section of a page goes through the codec
__device__ __forceinline__ bool pqw_coded(int codec, const PqFields& f) { return codec != kPqUncompressed && (uint32_t)f.usize > (uint32_t)f.def_len + (uint32_t)f.rep_len; }

// The plan, one lane per chunk.  In this order: more rows than 0xFFFFFFF0 (CJ_E_PARQUET_TABLE), in_len above 0x7E000000
// (CJ_E_INPUT_TOO_LARGE), the first row in page order that pq_row_fields refuses, a sum of the sizes that is not in_len.
__global__ __launch_bounds__(kBlockThreads) void pqw_plan_kernel(uint32_t n, int codec, const uint64_t* in_len, PqwTables t, PqwChunk* ch) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t np = t.count(i);
    int64_t err = np > 0xFFFFFFF0ull ? (int64_t)CJ_E_PARQUET_TABLE : in_len[i] > 0x7E000000ull ? (int64_t)CJ_E_INPUT_TOO_LARGE : 0;
    uint64_t sum = 0, nc = 0, slots = 0;
    const int64_t* w = t.rows(i);
    for (uint64_t k = 0; err == 0 && k < np; k++, w += kPqPageWords) {
        PqFields f;
        if ((err = pq_row_fields(w, f)) != 0) break;
        sum += (uint32_t)f.usize;
        if (pqw_coded(codec, f)) { nc++; slots += up16(pq_slot_bound(codec, (uint32_t)f.usize - (uint32_t)f.def_len - (uint32_t)f.rep_len)); }
    }
    if (err == 0 && sum != in_len[i]) err = CJ_E_PARQUET_TABLE;
    ch[i] = err ? PqwChunk{0, 0, 0, err, 0, 0, 0} : PqwChunk{0, 0, 0, 0, np, nc, slots};
}

// The rows of chunks [c0, c0 + nc), one lane per chunk: every page's place in the input, its table row copied — the kernels behind
// this one go by the copy alone —, and one encoder row per page the codec sees: its values into the next bound-sized slot, the slot
// offsets the running sum of the slot sizes.  The plan was made from the same table; should it have changed since, a row that no
// longer stands, that passes the chunk's length or that the plan's slots have no room for becomes an empty V1 page.
__global__ __launch_bounds__(kBlockThreads) void pqw_rows_kernel(uint32_t c0, uint32_t nc, int codec, const uint64_t* in_off, const uint64_t* in_len, PqwTables t,
                                                                 const PqwChunk* ch, PqwRows r) {
    const uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x;
    if (j >= nc) return;
    const uint32_t i = c0 + j;
    const PqwChunk f = ch[i];
    const int64_t* w = t.rows(i);
    uint64_t run = 0, kc = 0, slot = f.slot0;
    for (uint64_t k = 0; k < f.npages; k++, w += kPqPageWords) {
        const uint64_t g = f.page0 + k;
        int64_t row[kPqPageWords];
        for (size_t q = 0; q < kPqPageWords; q++) row[q] = w[q];
        PqFields p;
        bool ok = pq_row_fields(row, p) == 0 && run + (uint32_t)p.usize <= in_len[i];
        const uint64_t lv = (uint32_t)p.def_len + (uint32_t)p.rep_len, v = (uint32_t)p.usize - lv, cap = up16(pq_slot_bound(codec, v));
        bool coded = ok && pqw_coded(codec, p);
        if (coded && (kc >= f.ncoded || slot + cap > f.slot0 + f.slots)) ok = false;
        if (!ok) {
            for (size_t q = 0; q < kPqPageWords; q++) row[q] = 0;
            (void)pq_row_fields(row, p);
            coded = false;
        }
        for (size_t q = 0; q < kPqPageWords; q++) r.snap[kPqPageWords * g + q] = row[q];
        r.src[g] = in_off[i] + run; r.owner[g] = i; r.code[g] = kPqwNone; r.pay[g] = 0; r.crc[g] = 0; r.out[g] = kPqwNone;
        if (coded) {
            const uint64_t c = f.code0 + kc;
            r.code[g] = c;
            r.b.in_off[c] = in_off[i] + run + lv; r.b.in_len[c] = v; r.b.out_off[c] = slot; r.b.out_cap[c] = cap; r.b.result[c] = 0;
            slot += cap; kc++;
        }
        run += (uint32_t)p.usize;
    }
    // (an encoder row the walk no longer reaches: no input, no room — the encoder refuses it, nobody looks at its result)
    for (; kc < f.ncoded; kc++) {
        const uint64_t c = f.code0 + kc;
        r.b.in_off[c] = in_off[i]; r.b.in_len[c] = 0; r.b.out_off[c] = f.slot0; r.b.out_cap[c] = 0; r.b.result[c] = 0;
    }
}

// x^(8 n) mod P, for the combination of two CRCs: crc(A | B) = crc(A) * x^(8 |B|) + crc(B)
__device__ inline uint32_t pqw_xpow8(uint32_t n) {
    uint32_t p = 0x80000000u, b = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) p = gf_mul_ieee(p, b);
        b = gf_mul_ieee(b, b);
    }
    return p;
}

// the CRC-32 of p[0, len) by the whole wavefront, in every lane
__device__ __forceinline__ uint32_t pqw_wave_crc(const uint8_t* p, uint32_t len, const uint32_t* adv) {
    uint32_t c = crc32_lane(p, len, lane_id(), adv, d_pqw_crc32_tables.xpow8, [](const uint8_t* q) { return ld32u(q); });
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) c ^= __shfl_xor(c, sh, 64);
    return ~c;
}

// what the choice kernel decided for page g, for the two kernels behind it: the fields as they are written, where the values lie
struct PqwPage {
    PqFields f;
    uint32_t lv, vlen;
    const uint8_t *levels, *values;
};
__device__ __forceinline__ PqwPage pqw_page(const PqwRows& r, uint64_t g, const uint8_t* in_base, const uint8_t* slots) {
    PqwPage p;
    (void)pq_row_fields(r.snap + kPqPageWords * g, p.f);
    const int64_t pay = r.pay[g];
    p.lv = (uint32_t)p.f.def_len + (uint32_t)p.f.rep_len;
    p.f.csize = (int32_t)(uint32_t)pay; p.f.crc = (uint32_t)r.crc[g]; p.f.is_compressed = ((uint64_t)pay & kPqwCoded) != 0u;
    p.vlen = (uint32_t)p.f.csize - p.lv;
    p.levels = in_base + r.src[g];
    p.values = p.f.is_compressed ? slots + r.b.out_off[r.code[g]] : p.levels + p.lv;
    return p;
}

// One wavefront per page [p0, p0 + np): the codec's output or the raw values — a V2 page keeps the raw values (is_compressed = false)
// unless the output is shorter; a V1 or dictionary page has no such flag and carries the output, an encoder's code there is the
// page's —, and where the row asks for it the CRC-32 of the payload as it will be written: the levels in the input, then the values
// in the slot or in the input, the two spans' CRCs combined in GF(2).
__global__ __launch_bounds__(kBlockThreads) void pqw_choice_kernel(uint64_t p0, uint32_t np, const uint8_t* in_base, const uint8_t* slots, PqwRows r) {
    __shared__ uint32_t adv[1024];
    for (uint32_t i = threadIdx.x; i < 1024u; i += kBlockThreads) adv[i] = (&d_pqw_crc32_tables.adv256[0][0])[i];
    __syncthreads();
    const uint32_t j = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (j >= np) return;
    const uint64_t g = p0 + j;
    PqFields f;
    (void)pq_row_fields(r.snap + kPqPageWords * g, f);
    const uint32_t lv = (uint32_t)f.def_len + (uint32_t)f.rep_len, v = (uint32_t)f.usize - lv;
    const uint64_t c = r.code[g];
    uint32_t vlen = v;
    bool comp = false;
    if (c != kPqwNone) {
        const int64_t res = r.b.result[c];
        if (f.type == kPqDataPageV2) comp = res > 0 && res < (int64_t)v;
        else if (res <= 0 || res > (int64_t)r.b.out_cap[c]) {
            if (lane_id() == 0) r.pay[g] = res < 0 ? res : (int64_t)CJ_E_COMPRESS_FAILED;
            return;
        } else comp = true;
        if (comp) vlen = (uint32_t)res;
    }
    if (f.has_crc) {
        const uint8_t* levels = in_base + r.src[g];
        const uint8_t* values = comp ? slots + r.b.out_off[c] : levels + lv;
        uint32_t crc = pqw_wave_crc(values, vlen, adv);
        if (lv != 0u) {
            const uint32_t a = pqw_wave_crc(levels, lv, adv);
            crc = vlen != 0u ? gf_mul_ieee(a, pqw_xpow8(vlen)) ^ crc : a;
        }
        if (lane_id() == 0) r.crc[g] = crc;
    }
    if (lane_id() == 0) r.pay[g] = (int64_t)((uint64_t)(lv + vlen) | (comp ? kPqwCoded : 0u));
}

// One wavefront per chunk [c0, c0 + nc): the plan's code first; then the first page in page order with a code; then header plus
// payload of the pages in page order, 64 a round, a wave prefix sum carried across the rounds — a total above out_cap[i] is
// CJ_E_OUT_TOO_SMALL.  A chunk that stands gets every page's place in its slot; a refused one none: nothing of it is written.
__global__ __launch_bounds__(kBlockThreads) void pqw_layout_kernel(uint32_t c0, uint32_t nc, const PqwChunk* ch, PqwRows r, const uint8_t* in_base, const uint8_t* slots,
                                                                   const uint64_t* out_cap, int64_t* result) {
    const uint32_t j = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (j >= nc) return;
    const uint32_t i = c0 + j, lane = lane_id();
    const PqwChunk f = ch[i];
    int64_t err = f.err;
    uint64_t total = 0;
    const auto size_of = [&](uint64_t g) {
        const PqwPage p = pqw_page(r, g, in_base, slots);
        return pq_header_len(p.f) + (uint32_t)p.f.csize;
    };
    for (uint64_t b = 0; err == 0 && b < f.npages; b += 64u) {
        const bool in = b + lane < f.npages;
        const int64_t pay = in ? r.pay[f.page0 + b + lane] : 0;
        const uint64_t bad = ballot64(pay < 0);
        if (bad) { err = (int64_t)(int32_t)rdlane((uint32_t)pay, ctz64(bad)); break; }
        total += rdlane(wave_incl_scan(in ? size_of(f.page0 + b + lane) : 0u), 63);
    }
    if (err == 0 && total > out_cap[i]) err = CJ_E_OUT_TOO_SMALL;
    if (lane == 0) result[i] = err ? err : (int64_t)total;
    if (err != 0) return;                                       // (the rows kernel left every page of the chunk unplaced)
    uint64_t pos = 0;
    for (uint64_t b = 0; b < f.npages; b += 64u) {
        const bool in = b + lane < f.npages;
        const uint64_t g = f.page0 + b + lane;
        const uint32_t m = in ? size_of(g) : 0u;
        const uint32_t inc = wave_incl_scan(m);
        if (in) r.out[g] = pos + (inc - m);
        pos += rdlane(inc, 63);
    }
}

// One wavefront per page [p0, p0 + np) that has a place: lane 0 writes the header's bytes, then all lanes copy the levels from the
// input and the values from the slot or the input.  Every store lies in [the place, the place + header + payload), inside the
// chunk's total that the layout held to out_cap.
__global__ __launch_bounds__(kBlockThreads) void pqw_assemble_kernel(uint64_t p0, uint32_t np, PqwRows r, const uint8_t* in_base, const uint8_t* slots, uint8_t* out_base,
                                                                     const uint64_t* out_off) {
    const uint32_t j = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (j >= np) return;
    const uint64_t g = p0 + j, at = r.out[g];
    if (at == kPqwNone) return;
    const PqwPage p = pqw_page(r, g, in_base, slots);
    uint8_t* dst = out_base + out_off[r.owner[g]] + at;
    if (lane_id() == 0) pq_write_header(dst, p.f);
    dst += pq_header_len(p.f);
    wave_copy(dst, p.levels, p.lv);
    wave_copy(dst + p.lv, p.values, p.vlen);
}

}  // namespace cj

namespace {

using cj::PqwChunk;

// bytes of bound-sized page slots per turn of a compress batch at most; a chunk above it takes a turn alone
cj::SlotBudget g_slot_budget{256ull << 20};

struct Turn { size_t c0, c1; uint64_t p0, np, k0, nk; };     // chunks [c0, c1), their pages [p0, p0 + np) and encoder rows [k0, k0 + nk)

int pq_encode(cj_engine* e, int codec, size_t n, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, cj::PqwTables t, uint8_t* out_base,
              const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, hipStream_t s) {
    // One turn at the container batches' scratch, held across the call's one wait (cj_container.hpp)
    cj::ScratchTurn turn(e->fb, s);
    if (turn.rc != 0) return turn.rc;
    const size_t tab = cj::up16(n * sizeof(PqwChunk));
    int rc;
    if ((rc = turn.reserve(e->d_fb, tab)) != 0 || (rc = turn.reserve(e->h_fb, tab)) != 0) return rc;
    PqwChunk* h_ch = reinterpret_cast<PqwChunk*>(e->h_fb.p);
    hipLaunchKernelGGL(cj::pqw_plan_kernel, cj::lane_grid(n), dim3(cj::kBlockThreads), 0, s, (uint32_t)n, codec, in_len, t, reinterpret_cast<PqwChunk*>(e->d_fb.p));
    HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
    HIP_TRY(hipMemcpyAsync(h_ch, e->d_fb.p, n * sizeof(PqwChunk), hipMemcpyDeviceToHost, s), CJ_E_NO_DEVICE);
    HIP_TRY(hipStreamSynchronize(s), CJ_E_NO_DEVICE);       // the one wait: the host sizes the rows and cuts the turns from the chunks' plans
    // the scan, and turns of whole chunks under the slot budget
    // (a batch above the budget is cut into turns of about equal size: a last turn of a few chunks would cost a whole encoder launch)
    uint64_t all = 0;
    for (size_t i = 0; i < n; i++) all += h_ch[i].slots;
    const uint64_t limit = g_slot_budget.load(), parts = std::max<uint64_t>(1, (all + limit - 1) / limit), budget = std::min(limit, all / parts + 1);
    std::vector<Turn> turns;
    uint64_t nb = 0, nk = 0, fill = 0, most = 0;
    Turn cur{0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        const uint64_t need = h_ch[i].slots;
        if (cur.c1 > cur.c0 && fill + need > budget) { turns.push_back(cur); cur = Turn{i, i, nb, 0, nk, 0}; fill = 0; }
        h_ch[i].page0 = nb; h_ch[i].code0 = nk; h_ch[i].slot0 = fill;
        nb += h_ch[i].npages; nk += h_ch[i].ncoded; fill += need;
        cur.c1 = i + 1; cur.np += h_ch[i].npages; cur.nk += h_ch[i].ncoded;
        most = std::max(most, fill);
    }
    turns.push_back(cur);
    if (nb > 0xFFFFFFF0ull) return CJ_E_BAD_ARG;
    const size_t o_slots = cj::up16(tab + 8 * (cj::kPqwRowWords * (size_t)nb + cj::kBatchRowWords * (size_t)nk));
    if ((rc = turn.reserve(e->d_fb, o_slots + (size_t)most + 16)) != 0) return rc;
    uint8_t* d = (uint8_t*)e->d_fb.p;
    PqwChunk* ch = reinterpret_cast<PqwChunk*>(d);
    uint8_t* slots = d + o_slots;
    const cj::PqwRows r = cj::pqw_rows(reinterpret_cast<uint64_t*>(d + tab), (size_t)nb, (size_t)nk);
    HIP_TRY(hipMemcpyAsync(ch, h_ch, n * sizeof(PqwChunk), hipMemcpyHostToDevice, s), CJ_E_NO_DEVICE);
    for (const Turn& u : turns) {
        const uint32_t c0 = (uint32_t)u.c0, nc = (uint32_t)(u.c1 - u.c0), np = (uint32_t)u.np;
        if (np) hipLaunchKernelGGL(cj::pqw_rows_kernel, cj::lane_grid(nc), dim3(cj::kBlockThreads), 0, s, c0, nc, codec, in_off, in_len, t, ch, r);
        // lock order: fb, then the encoder's slots (cj_engine.hpp)
        if (u.nk && (rc = cj::inner_encode(e, cj::pq_inner(codec), in_base, slots, r.b.sub((size_t)u.k0, (size_t)u.nk), (uint32_t)u.nk, s)) != 0) return rc;
        if (np) hipLaunchKernelGGL(cj::pqw_choice_kernel, cj::wave_grid(np), dim3(cj::kBlockThreads), 0, s, u.p0, np, in_base, slots, r);
        hipLaunchKernelGGL(cj::pqw_layout_kernel, cj::wave_grid(nc), dim3(cj::kBlockThreads), 0, s, c0, nc, ch, r, in_base, slots, out_cap, result);
        if (np) hipLaunchKernelGGL(cj::pqw_assemble_kernel, cj::wave_grid(np), dim3(cj::kBlockThreads), 0, s, u.p0, np, r, in_base, slots, out_base, out_off);
    }
    return turn.done(s);
}

bool args_ok(int what, uint32_t flags) { return cj::pq_codec_ok(what) && flags == 0u; }

}  // namespace

extern "C" {

size_t cj_parquet_compress_bound(int what, size_t n_bytes, size_t n_pages) {
    return (!cj::pq_codec_ok(what) || n_bytes > 0x7E000000ull || n_pages > 0xFFFFFFF0ull) ? 0 : (size_t)cj::pq_chunk_bound(what, n_bytes, n_pages);
}

int cj_parquet_compress_device(cj_engine* e, int what, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                               const int64_t* rows, const uint64_t* row_off, const uint64_t* row_cnt, uint8_t* out_base, const uint64_t* out_off,
                               const uint64_t* out_cap, int64_t* result, void* hip_stream) {
    if (!args_ok(what, flags)) return CJ_E_BAD_ARG;
    return cj::device_call(e, n_chunks, {in_base, in_off, in_len, rows, row_off, row_cnt, out_base, out_off, out_cap, result}, hip_stream, [&](cj_engine* e, hipStream_t s) {
        const cj::PqwTables t{reinterpret_cast<const uint8_t*>(rows), row_off, row_cnt, 8u * (uint32_t)cj::kPqPageWords, 1u};
        return pq_encode(e, what, n_chunks, in_base, in_off, in_len, t, out_base, out_off, out_cap, result, s);
    });
}

int cj_parquet_compress_host(cj_engine* e, int what, uint32_t flags, size_t n, const uint8_t* const* in_ptrs, const size_t* in_lens, const int64_t* const* rows_ptrs,
                             const size_t* row_cnts, uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result) {
    if (!args_ok(what, flags)) return CJ_E_BAD_ARG;
    const int g = cj::batch_gate(n, {in_ptrs, in_lens, rows_ptrs, row_cnts, out_ptrs, out_caps, result});
    if (g != cj::kBatchGo) return g;
    // The tables are staged as n more inputs of the same host batch, behind the chunks: entry n + i is chunk i's table, and has no
    // output.  A table of more rows than a batch can have is refused here (CJ_E_PARQUET_TABLE) and travels as an empty chunk.
    constexpr size_t kRow = 8 * cj::kPqPageWords;
    if (n > 0x7FFFFFF0ull) return CJ_E_BAD_ARG;
    std::vector<const uint8_t*> ins(2 * n, nullptr);
    std::vector<uint8_t*> outs(2 * n, nullptr);
    std::vector<size_t> lens(2 * n, 0), caps(2 * n, 0);
    std::vector<int64_t> res(2 * n, 0);
    for (size_t i = 0; i < n; i++) {
        if (row_cnts[i] > 0xFFFFFFF0ull) continue;
        if (row_cnts[i] > (size_t)0x7E000000u / kRow) return CJ_E_BAD_ARG;
        ins[i] = in_ptrs[i]; lens[i] = in_lens[i]; outs[i] = out_ptrs[i]; caps[i] = out_caps[i];
        ins[n + i] = reinterpret_cast<const uint8_t*>(rows_ptrs[i]); lens[n + i] = row_cnts[i] * kRow;
    }
    const int rc = cj::host_call(e, 2 * n, ins.data(), lens.data(), outs.data(), caps.data(), res.data(), -1, false,
                                 [&](cj_engine* e, const uint8_t* d_in, uint8_t* d_out, const cj::BatchRows& d, hipStream_t s) {
        HIP_TRY(hipMemsetAsync(d.result + n, 0, 8 * n, s), CJ_E_NO_DEVICE);
        const cj::PqwTables t{d_in, d.in_off + n, d.in_len + n, 1u, (uint32_t)kRow};
        return pq_encode(e, what, n, d_in, d.in_off, d.in_len, t, d_out, d.out_off, d.out_cap, d.result, s);
    });
    if (rc != 0) return rc;
    for (size_t i = 0; i < n; i++) result[i] = row_cnts[i] > 0xFFFFFFF0ull ? (int64_t)CJ_E_PARQUET_TABLE : res[i];
    return 0;
}

// tests: the bytes of page slots per turn of a Parquet compress batch (0 = the default); returns the previous value
uint64_t cj_debug_parquet_slot_budget(uint64_t bytes) { return g_slot_budget.exchange(bytes); }

}  // extern "C"
