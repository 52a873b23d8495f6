// zstd_enc_wave.hpp — the entropy stage of the Zstandard encoder, one wavefront per frame: the sequence records that
// the matcher left in the workgroup's scratch slot become one block per piece — RLE, Compressed or Raw by their exact sizes — behind
// the frame header.  tests/hostsim/zstd_enc_model.c states the same thing as scalar C; this text emits exactly its bytes.  Written
// like deflate_enc_wave.hpp, whose code builder (dfe_build_lens), bit writer (dfe_put, dfe_put_round, dfe_flush_bytes) and LDS block
// it uses as they are: it names only
//     wave_copy, wave_order, CJ_LANES, LaneU32, LaneU64, lane_excl_add, lds_ld, lds_ld8, lds_add, lds_or, in_ld8, in_ld32, out_st8, out_st32
// of the wave-decoder contract, and what whoever includes this declares:
//     rec_ld(slot, i)             record i of the scratch slot
//     rec_st32(slot, i, w, v)     word w of record i
//     lit_ld8(p) / lit_st8(p, v)  a byte of the slot's literal area (a wave_copy's source as well)
// Not part of the C-ABI.
//
// Mapping.  Block type, modes and sizes are wave-uniform.  The lanes take consecutive records, literals or sequences:
//   scan      64 records a round: the records must tile the piece (else the block is Raw: nothing below relies on the matcher), the
//             LL / OF / ML codes of the sequences go into three LDS histograms, the extra bits are summed
//   gather    a prefix sum over the records' literal counts gives every literal its source position (the six-step search of §5.13);
//             the literals go into the slot's literal area, in order
//   literals  byte histogram, the §5.13 builder at limit 11, weights and codes in libzstd's order (by weight, then by symbol), the tree
//             as direct or FSE-compressed weights (lane 0: zstd_fse_enc.h), the sizes of the quarters' streams from one pass over the
//             literals; then Raw or Huffman by exact size
//   tables    lanes 0 / 1 / 2 normalise the LL / OF / ML histograms, write their NCount, compare FSE_Compressed with Predefined by an
//             integer cost and build the encode tables (state table, deltaNbBits, deltaFindState): zstd_fse_enc.h, the model's text too
//   pass A    the state chains are serial: lanes 0 / 1 / 2 walk LL / OF / ML from the last sequence to the first, 64 sequences a
//             round out of LDS, and leave (bit count, bits) of every state flush in the upper 15 bits of the record's words 0 / 1 / 2
//             (the words hold values up to 65 536: 17 bits)
//   pass B    now every sequence's bit count is known: two lanes a sequence (state bits + LL extra | ML extra + OF extra), a prefix
//             sum gives the offsets, the §5.13 bit writer ORs them into LDS and stores whole dwords
// The block's exact size is known before its first store.  Every loop is bounded by the piece's length, the record count or an
// alphabet's size; every index into LDS or the slot is masked or compared.
#pragma once
#include "deflate_enc_wave.hpp"
#define ZSF_FN __device__ __forceinline__
#include "zstd_fse_enc.h"

namespace cj {

constexpr uint32_t kZsePiece = kDfePiece;
constexpr uint32_t kZseSlotRecs = kDfeSlotRecs;
constexpr uint32_t kZseRecBytes = (kZseSlotRecs * 16u + 255u) & ~255u;
constexpr uint32_t kZseSlotBytes = kZseRecBytes + kZsePiece;        // the records, then the piece's gathered literals
constexpr uint32_t kZseInMax = 0x7E000000u;
constexpr uint32_t kZseChecksum = 1u;                                // CJ_ZSTD_FLAG_CHECKSUM
constexpr uint32_t kZseLL = 0u, kZseOF = 40u, kZseML = 72u;           // the three code histograms inside ZseLds::sh
constexpr uint32_t kZseInfo = 10u;      // words of a piece's report: 0 literal mode, 1 streams, 2 tree kind, 3 / 4 / 5 LL / OF / ML mode, 6 sequences, 7 literals, 8 bits in the last byte, 9 block type

// The wavefront's LDS: DfeLds (11.3 KiB) + 7.0 KiB
struct ZseLds {
    DfeLds d;                // hist / lens / code: the literals' alphabet; the code builder's arrays (key .. iw double as the table builder's cells and sums); stage; rl, pre
    uint32_t sh[128];        // code counts: LL at 0, OF at 40, ML at 72
    uint16_t st[1344];       // the state tables: LL at 0 (512), OF at 512 (256), ML at 768 (512), the Huffman weights' at 1280 (64)
    uint32_t dnb[256];       // deltaNbBits, 64 a table (the weights' is table 3)
    int32_t dfs[256];        // deltaFindState
    int16_t nrm[256];        // normalized counts, 64 a table
    uint32_t tb[12];         // table t: mode (0 Predefined, 1 RLE, 2 FSE_Compressed) at t, accuracy log at 4 + t, bytes of its description at 8 + t; [3]: bytes of the FSE-compressed weights (0: none)
    uint32_t wh[16];         // the weights' histogram
    uint8_t nc[3][96];       // the tables' descriptions (NCount)
    uint8_t wt[256];         // the Huffman weights
    uint8_t wout[224];       // their FSE-compressed form
    uint16_t rr[3][64];      // pass A: a round's (bit count << 9 | bits) per table
    uint8_t rc[3][64];       // ... and its codes
    uint32_t acc[16];        // 0 the records do not tile the piece, 1 literals, 2 extra bits, 3 state bits, 4 .. 7 bits of the literal streams, 8 .. 10 codes used, 11 .. 13 the final states, 14 the piece is not one byte repeated
};

struct ZseOut { uint8_t* out; uint32_t cap, op; };      // op bytes of the frame are written

__device__ __forceinline__ void zse_ll(uint32_t v, uint32_t& c, uint32_t& bits, uint32_t& base) {      // v <= 65536
    if (v < 16u) { c = v; bits = 0u; base = v; }
    else if (v < 24u) { c = 16u + ((v - 16u) >> 1); bits = 1u; base = 16u + 2u * (c - 16u); }
    else if (v < 32u) { c = 20u + ((v - 24u) >> 2); bits = 2u; base = 24u + 4u * (c - 20u); }
    else if (v < 48u) { c = 22u + ((v - 32u) >> 3); bits = 3u; base = 32u + 8u * (c - 22u); }
    else if (v < 64u) { c = 24u; bits = 4u; base = 48u; }
    else { bits = dfe_ilog2(v); c = bits + 19u; base = 1u << bits; }
}
// a match length (3 <= v <= 65536): its code, extra bits and the first length of the code
__device__ __forceinline__ void zse_ml(uint32_t v, uint32_t& c, uint32_t& bits, uint32_t& base) {
    const uint32_t m = v - 3u;
    if (m < 32u) { c = m; bits = 0u; base = v; return; }
    uint32_t b;
    if (m < 40u) { c = 32u + ((m - 32u) >> 1); bits = 1u; b = 32u + 2u * (c - 32u); }
    else if (m < 48u) { c = 36u + ((m - 40u) >> 2); bits = 2u; b = 40u + 4u * (c - 36u); }
    else if (m < 64u) { c = 38u + ((m - 48u) >> 3); bits = 3u; b = 48u + 8u * (c - 38u); }
    else if (m < 96u) { c = 40u + ((m - 64u) >> 4); bits = 4u; b = 64u + 16u * (c - 40u); }
    else if (m < 128u) { c = 42u; bits = 5u; b = 96u; }
    else { bits = dfe_ilog2(m); c = bits + 36u; b = 1u << bits; }
    base = b + 3u;
}
// Offset_Value: distance + 3, or the repeat code 1 (a literal length above 0 and the distance of the frame's previous sequence)
__device__ __forceinline__ uint32_t zse_ofv(uint32_t lit, uint32_t dist, uint32_t before) { return lit != 0u && dist == before ? 1u : dist + 3u; }

// the predefined distributions (RFC 8878 3.1.1.3.2.2; -1: "less than one")
__device__ __forceinline__ int32_t zse_default_norm(uint32_t which, uint32_t s) {
    static const int8_t kLL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    static const int8_t kOF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    static const int8_t kML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    return which == 0u ? kLL[s < 36u ? s : 35u] : which == 1u ? kOF[s < 29u ? s : 28u] : kML[s < 53u ? s : 52u];
}
__device__ __forceinline__ uint32_t zse_st_at(uint32_t t) { return t == 0u ? 0u : t == 1u ? 512u : 768u; }
__device__ __forceinline__ uint32_t zse_default_log(uint32_t t) { return t == 1u ? 5u : 6u; }
__device__ __forceinline__ uint32_t zse_default_syms(uint32_t t) { return t == 0u ? 36u : t == 1u ? 29u : 53u; }

__device__ __forceinline__ void zse_bytes(uint8_t* p, uint64_t v, uint32_t k) {       // k <= 8 bytes of v, little-endian
    CJ_LANES(lane) { if (lane < k) out_st8(p + lane, (uint32_t)(v >> (8u * lane)) & 0xffu); }
    wave_order();
}

__device__ __forceinline__ uint32_t zse_max_log(uint32_t t) { return t == 1u ? 8u : 9u; }
// One lane's work: table t (0 .. 2 the sequences', 3 the weights') of L->nrm's counts into L->st / dnb / dfs; cells and sums in the code builder's arrays
__device__ __forceinline__ void zse_table(ZseLds* L, uint32_t t, uint32_t log, uint32_t nsym) {
    t &= 3u;
    zsf_table(L->nrm + 64u * t, nsym < 64u ? nsym : 64u, log < 9u ? log : 9u, L->st + (t == 3u ? 1280u : zse_st_at(t)), L->dnb + 64u * t, L->dfs + 64u * t,
              reinterpret_cast<uint8_t*>(L->d.key) + 512u * t, L->d.iw + 72u * t);      // (key and sw: 2304 bytes; iw: 288 words)
}
// ... with its predefined distribution
__device__ __forceinline__ void zse_build_table(ZseLds* L, uint32_t t) {
    const uint32_t nsym = zse_default_syms(t);
    for (uint32_t s = 0; s < nsym; s++) L->nrm[64u * t + s] = (int16_t)zse_default_norm(t, s);
    zse_table(L, t, zse_default_log(t), nsym);
}
// One lane's work: the mode of table t from its histogram hist[0, m) of nseq codes — RLE is the caller's; FSE_Compressed when its
// estimated bits (1 / 256 bit a unit: the description's exact bits and every code's cost from its normalized count) are below the
// predefined distribution's; else Predefined — and the table
__device__ __forceinline__ void zse_choose_table(ZseLds* L, uint32_t t, const uint32_t* hist, uint32_t m, uint32_t nseq) {
    uint32_t used = 0, top = 0, pre = 0, fse;
    for (uint32_t c = 0; c < m; c++) if (hist[c] != 0u) { used++; top = c; }
    const uint32_t flog = zsf_pick_log(zse_max_log(t), used, nseq);
    zsf_normalise(hist, top + 1u, nseq, flog, L->nrm + 64u * t);
    const uint32_t ncb = zsf_ncount(L->nrm + 64u * t, top + 1u, flog, L->nc[t], 96u);
    fse = ncb * 8u * 256u;
    for (uint32_t c = 0; c <= top; c++) {
        const uint32_t h = hist[c];
        if (h == 0u) continue;
        const int32_t d = zse_default_norm(t, c);
        fse += h * zsf_cost((uint32_t)L->nrm[64u * t + c], flog);
        pre += h * zsf_cost((uint32_t)(d < 0 ? 1 : d), zse_default_log(t));
    }
    if (fse < pre && ncb <= 96u) { L->tb[t] = 2u; L->tb[4u + t] = flog; L->tb[8u + t] = ncb; zse_table(L, t, flog, top + 1u); }
    else { L->tb[t] = 0u; L->tb[4u + t] = zse_default_log(t); L->tb[8u + t] = 0u; zse_build_table(L, t); }
}

// the literals header of a Raw (0) or RLE (1) section: its length; written at p when p is not null
__device__ __forceinline__ uint32_t zse_lit_plain(uint8_t* p, uint32_t type, uint32_t n) {
    const uint32_t len = n <= 31u ? 1u : n <= 4095u ? 2u : 3u;
    if (p) zse_bytes(p, len == 1u ? (type | n << 3) : len == 2u ? (type | 1u << 2 | n << 4) : (type | 3u << 2 | n << 4), len);
    return len;
}

// literals [a, b) of lit, the last one first, as one Huffman stream at p; returns its length
__device__ __forceinline__ uint32_t zse_huf_stream(ZseLds* L, uint8_t* p, const uint8_t* lit, uint32_t a, uint32_t b) {
    DfeOut W;
    dfe_out_init(&L->d, W, p, 0u);
    for (uint32_t s0 = a; s0 < b; s0 += 64u) {
        LaneU64 val;
        LaneU32 nb;
        CJ_LANES(lane) {
            nb[lane] = 0u; val[lane] = 0ull;
            if (s0 + lane < b) {
                const uint32_t c = L->d.code[lit_ld8(lit + (b - 1u - (s0 - a) - lane)) & 255u];
                val[lane] = c & 0xffffu; nb[lane] = c >> 16;
            }
        }
        dfe_put_round(&L->d, W, val, nb);
    }
    dfe_put(&L->d, W, 1u, 1u);
    dfe_flush_bytes(&L->d, W);
    return W.obyte;
}

// One piece (pn <= 65536 bytes at in, its nrec records at slot, `lit`: the slot's literal area) as one block at O.op; `last` sets
// Last_Block.  tail: bytes the frame still needs behind its last block.  prev: the distance of the frame's previous sequence, advanced
// by a Compressed block only.  Returns false, before the block's first store, when the block (and the tail) does not fit the capacity.
// info (may be null): kZseInfo words
__device__ __forceinline__ bool zse_piece(ZseLds* L, ZseOut& O, const uint8_t* in, uint32_t pn, DfeRec* slot, uint32_t nrec, uint8_t* lit, bool last,
                                          uint32_t tail, uint32_t& prev, uint32_t* info) {
    DfeLds* D = &L->d;
    CJ_LANES(lane) {
        L->sh[lane] = 0u; L->sh[64u + lane] = 0u;
        if (lane < 16u) L->acc[lane] = 0u;
        for (uint32_t s = lane; s < 320u; s += 64u) { D->hist[s] = 0u; D->lens[s] = 0u; D->code[s] = 0u; }
    }
    wave_order();
    // ---- is the piece one byte repeated (4 KiB a turn; a text leaves in the first)
    const uint32_t b0 = pn ? in_ld8(in) : 0u;
    for (uint32_t at = 0; at < pn; at += 4096u) {
        CJ_LANES(lane) {
            uint32_t diff = 0;
            for (uint32_t k = at + lane; k < pn && k < at + 4096u; k += 64u) diff |= in_ld8(in + k) ^ b0;
            if (diff) lds_or(&L->acc[14], 1u);
        }
        wave_order();
        if (lds_ld(&L->acc[14]) != 0u) break;
    }
    const bool same = pn != 0u && lds_ld(&L->acc[14]) == 0u;
    // ---- scan: the records tile the piece; the sequences' codes counted
    const bool sane = nrec != 0u && nrec <= kZseSlotRecs && !same;
    for (uint32_t r0 = 0; sane && r0 < nrec; r0 += 64u) {
        CJ_LANES(lane) {
            const uint32_t i = r0 + lane;
            if (i < nrec) {
                const DfeRec q = rec_ld(slot, i);
                uint32_t at = 0, before = prev;
                if (i != 0u) { const DfeRec p = rec_ld(slot, i - 1u); at = p.lit0 + p.lit + p.mlen; before = p.dist; }
                bool ok = q.lit0 == at && q.lit0 <= pn && q.lit <= pn - q.lit0;
                const uint32_t e = q.lit0 + q.lit;
                if (i + 1u == nrec) ok = ok && q.mlen == 0u && e == pn;
                else ok = ok && q.mlen >= 3u && q.mlen <= pn - e && q.dist >= 1u && q.dist <= e && q.dist <= 65535u;
                if (!ok) lds_or(&L->acc[0], 1u);
                else {
                    if (q.lit != 0u) lds_add(&L->acc[1], q.lit);
                    if (i + 1u != nrec) {
                        uint32_t lc, lb, mc, mb, base;
                        zse_ll(q.lit, lc, lb, base);
                        zse_ml(q.mlen, mc, mb, base);
                        const uint32_t oc = dfe_ilog2(zse_ofv(q.lit, q.dist, before));
                        lds_add(&L->sh[kZseLL + (lc < 36u ? lc : 35u)], 1u);
                        lds_add(&L->sh[kZseOF + (oc & 31u)], 1u);
                        lds_add(&L->sh[kZseML + (mc < 53u ? mc : 52u)], 1u);
                        lds_add(&L->acc[2], lb + mb + oc);
                    }
                }
            }
        }
        wave_order();
    }
    const bool tiled = sane && lds_ld(&L->acc[0]) == 0u;
    const uint32_t nseq = tiled ? nrec - 1u : 0u, nlit = tiled ? (lds_ld(&L->acc[1]) < kZsePiece ? lds_ld(&L->acc[1]) : kZsePiece) : 0u;
    uint32_t type = same ? 1u : 0u, size = same ? 1u : pn;
    uint32_t lmode = 0, streams = 0, lsize = 0, maxlen = 0, top = 0, lhl = 0, seg = 0, seq_bits = 0, rle_mask = 0, rle_sym[3] = {0u, 0u, 0u}, kind = 0, desc = 0, wfse = 0, tlog[3] = {0u, 0u, 0u}, tmode[3] = {0u, 0u, 0u}, tncb[3] = {0u, 0u, 0u};
    if (tiled) {
        // ---- gather the literals
        uint32_t base = 0;
        for (uint32_t r0 = 0; r0 < nrec; r0 += 64u) {
            LaneU32 ns, before;
            CJ_LANES(lane) {
                DfeRec q = {0u, 0u, 1u, 0u};
                if (r0 + lane < nrec) q = rec_ld(slot, r0 + lane);
                if (q.lit0 > pn) q.lit0 = pn;
                if (q.lit > pn - q.lit0) q.lit = pn - q.lit0;
                D->rl[lane] = q;
                ns[lane] = q.lit;
            }
            const uint32_t total = lane_excl_add(ns, before);
            CJ_LANES(lane) { D->pre[lane] = before[lane]; }
            wave_order();
            for (uint32_t s0 = 0; s0 < total; s0 += 64u) {
                CJ_LANES(lane) {
                    const uint32_t k = s0 + lane;
                    if (k < total && base + k < nlit) {
                        uint32_t r = 0;
                        for (uint32_t step = 32u; step != 0u; step >>= 1) if (D->pre[(r + step) & 63u] <= k) r += step;
                        const DfeRec q = D->rl[r & 63u];
                        const uint32_t j = k - D->pre[r & 63u];
                        const uint32_t b = j < q.lit ? in_ld8(in + q.lit0 + j) : 0u;
                        lit_st8(lit + base + k, b);
                        lds_add(&D->hist[b & 255u], 1u);
                    }
                }
            }
            wave_order();
            base += total;
        }
        // ---- the literals section: Raw or Huffman (one distinct literal is one distinct byte while the pieces are independent: an RLE block)
        const uint32_t raw = zse_lit_plain(nullptr, 0u, nlit) + nlit;
        lsize = raw;
        dfe_build_lens(D, D->hist, 256u, 11u, false, D->lens);
        const uint32_t used = lds_ld(&D->acc[0]);
        top = 255u;
        while (top != 0u && lds_ld(&D->hist[top]) == 0u) top--;
        if (used >= 2u) {
            maxlen = 11u;
            while (maxlen > 1u && lds_ld(&D->blc[maxlen]) == 0u) maxlen--;
            // the tree: direct 4-bit weights (at most 128 of them) or FSE-compressed weights (one lane's work), whichever is smaller
            CJ_LANES(lane) {
                for (uint32_t s = lane; s < 256u; s += 64u) { const uint32_t l = D->lens[s]; L->wt[s] = (uint8_t)(l != 0u && l <= maxlen ? maxlen + 1u - l : 0u); }
            }
            wave_order();
            CJ_LANES(lane) {
                if (lane == 0u)
                    L->tb[3] = zsf_weights(L->wt, top, L->wout, 224u, L->wh, L->nrm + 192u, L->st + 1280u, L->dnb + 192u, L->dfs + 192u,
                                           reinterpret_cast<uint8_t*>(D->key) + 1536u, D->iw + 216u);
            }
            wave_order();
            wfse = lds_ld(&L->tb[3]) < 128u ? lds_ld(&L->tb[3]) : 0u;
            if (top <= 128u) { desc = 1u + (top + 1u) / 2u; kind = 1u; }
            if (wfse != 0u && (kind == 0u || 1u + wfse < desc)) { desc = 1u + wfse; kind = 2u; }
        }
        if (kind != 0u) {
            streams = nlit <= 1023u ? 1u : 4u;
            seg = streams == 1u ? nlit : (nlit + 3u) / 4u;
            CJ_LANES(lane) {
                uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                for (uint32_t i = lane; i < nlit; i += 64u) {
                    const uint32_t l = D->lens[lit_ld8(lit + i) & 255u];
                    const uint32_t q = i / (seg ? seg : 1u);
                    s0 += q == 0u ? l : 0u; s1 += q == 1u ? l : 0u; s2 += q == 2u ? l : 0u; s3 += q >= 3u ? l : 0u;
                }
                if (s0) lds_add(&L->acc[4], s0);
                if (s1) lds_add(&L->acc[5], s1);
                if (s2) lds_add(&L->acc[6], s2);
                if (s3) lds_add(&L->acc[7], s3);
            }
            wave_order();
            lhl = nlit <= 1023u ? 3u : nlit <= 16383u ? 4u : 5u;
            uint32_t total = lhl + desc + (streams == 4u ? 6u : 0u);
            for (uint32_t q = 0; q < streams; q++) total += (lds_ld(&L->acc[4u + q]) + 8u) >> 3;
            if (total < lsize) { lsize = total; lmode = 2u; }
        }
        // ---- the sequences section
        uint32_t qsize = nseq < 128u ? 1u : 2u;
        if (nseq != 0u) {
            CJ_LANES(lane) {
                if (lane < 56u) {
                    if (lane < 36u && L->sh[kZseLL + lane] != 0u) lds_add(&L->acc[8], 1u);
                    if (lane < 32u && L->sh[kZseOF + lane] != 0u) lds_add(&L->acc[9], 1u);
                    if (L->sh[kZseML + lane] != 0u) lds_add(&L->acc[10], 1u);
                }
            }
            wave_order();
            for (uint32_t t = 0; t < 3u; t++) {
                if (lds_ld(&L->acc[8u + t]) != 1u) continue;
                rle_mask |= 1u << t;
                const uint32_t at = t == 0u ? kZseLL : t == 1u ? kZseOF : kZseML, m = t == 0u ? 36u : t == 1u ? 32u : 56u;
                uint32_t s = 0;
                while (s + 1u < m && lds_ld(&L->sh[at + s]) == 0u) s++;
                rle_sym[t] = s;
            }
            CJ_LANES(lane) {
                if (lane < 3u) {
                    if ((rle_mask >> lane) & 1u) { L->tb[lane] = 1u; L->tb[4u + lane] = 0u; L->tb[8u + lane] = 1u; }
                    else zse_choose_table(L, lane, L->sh + (lane == 0u ? kZseLL : lane == 1u ? kZseOF : kZseML), lane == 0u ? 36u : lane == 1u ? 32u : 53u, nseq);
                }
            }
            wave_order();
            for (uint32_t t = 0; t < 3u; t++) {
                tmode[t] = lds_ld(&L->tb[t]) & 3u;
                tlog[t] = lds_ld(&L->tb[4u + t]) < 9u ? lds_ld(&L->tb[4u + t]) : 9u;
                tncb[t] = lds_ld(&L->tb[8u + t]) < 96u ? lds_ld(&L->tb[8u + t]) : 96u;
            }
            // pass A: the state chains, from the last sequence to the first
            LaneU32 state;
            CJ_LANES(lane) { state[lane] = 0u; }
            for (uint32_t done = 0; done < nseq; done += 64u) {
                const uint32_t hi = nseq - done, cnt = hi < 64u ? hi : 64u;
                LaneU32 w0, w1, w2;
                CJ_LANES(lane) {
                    w0[lane] = 0u; w1[lane] = 0u; w2[lane] = 0u;
                    L->rr[0][lane] = 0u; L->rr[1][lane] = 0u; L->rr[2][lane] = 0u;
                    L->rc[0][lane] = 0u; L->rc[1][lane] = 0u; L->rc[2][lane] = 0u;
                    if (lane < cnt) {
                        const uint32_t i = hi - 1u - lane;
                        const DfeRec q = rec_ld(slot, i);
                        const uint32_t before = i != 0u ? rec_ld(slot, i - 1u).dist & 0x1ffffu : prev;
                        uint32_t lc, mc, bits, base;
                        zse_ll(q.lit, lc, bits, base);
                        zse_ml(q.mlen, mc, bits, base);
                        L->rc[0][lane] = (uint8_t)(lc < 36u ? lc : 35u);
                        L->rc[1][lane] = (uint8_t)(dfe_ilog2(zse_ofv(q.lit, q.dist, before)) & 31u);
                        L->rc[2][lane] = (uint8_t)(mc < 53u ? mc : 52u);
                        w0[lane] = q.lit0; w1[lane] = q.lit; w2[lane] = q.dist;
                    }
                }
                wave_order();
                CJ_LANES(lane) {
                    if (lane < 3u && !((rle_mask >> lane) & 1u)) {
                        const uint32_t log = L->tb[4u + lane] < 9u ? L->tb[4u + lane] : 9u, mask = (1u << log) - 1u;
                        const uint16_t* st = L->st + zse_st_at(lane);
                        uint32_t s = state[lane], sum = 0;
                        for (uint32_t k = 0; k < cnt; k++) {
                            const uint32_t sym = L->rc[lane][k] & 63u, dnb = L->dnb[64u * lane + sym];
                            const int32_t dfs = L->dfs[64u * lane + sym];
                            if (done == 0u && k == 0u) {                       // the last sequence opens the state and leaves no bits
                                const uint32_t nb = (dnb + (1u << 15)) >> 16, v = (nb << 16) - dnb;
                                s = st[(uint32_t)((int32_t)(v >> nb) + dfs) & mask];
                            } else {
                                const uint32_t nb = ((s + dnb) >> 16) & 15u;
                                L->rr[lane][k] = (uint16_t)(nb << 9 | (s & ((1u << nb) - 1u)));
                                sum += nb;
                                s = st[(uint32_t)((int32_t)(s >> nb) + dfs) & mask];
                            }
                        }
                        state[lane] = s;
                        lds_add(&L->acc[3], sum);
                        L->acc[11u + lane] = s;
                    }
                }
                wave_order();
                CJ_LANES(lane) {
                    if (lane < cnt) {
                        const uint32_t i = hi - 1u - lane;
                        rec_st32(slot, i, 0u, w0[lane] | (uint32_t)L->rr[0][lane] << 17);
                        rec_st32(slot, i, 1u, w1[lane] | (uint32_t)L->rr[1][lane] << 17);
                        rec_st32(slot, i, 2u, w2[lane] | (uint32_t)L->rr[2][lane] << 17);
                    }
                }
                wave_order();
            }
            seq_bits = lds_ld(&L->acc[2]) + lds_ld(&L->acc[3]) + 1u;
            for (uint32_t t = 0; t < 3u; t++) seq_bits += tlog[t];
            qsize += 1u + tncb[0] + tncb[1] + tncb[2] + ((seq_bits + 7u) >> 3);
        }
        if (lsize + qsize < pn) { type = 2u; size = lsize + qsize; }
    }
    if (info) {
        for (uint32_t k = 0; k < kZseInfo; k++) info[k] = 0u;
        info[9] = type;
        if (type == 2u) {
            info[0] = lmode; info[1] = lmode == 2u ? streams : 0u; info[2] = lmode == 2u ? kind : 0u;
            info[3] = tmode[0]; info[4] = tmode[1]; info[5] = tmode[2]; info[6] = nseq; info[7] = nlit;
            info[8] = nseq ? (seq_bits - 1u) & 7u : 0u;
        }
    }
    // ---- the block: nothing was stored so far
    if ((uint64_t)O.op + 3u + size + (last ? tail : 0u) > O.cap) return false;
    zse_bytes(O.out + O.op, (last ? 1u : 0u) | type << 1 | (type == 2u ? size : pn) << 3, 3u);
    O.op += 3u;
    if (type == 0u) { wave_copy(O.out + O.op, in, pn); O.op += pn; return true; }
    if (type == 1u) { zse_bytes(O.out + O.op, b0, 1u); O.op += 1u; return true; }
    uint8_t* p = O.out + O.op;
    if (lmode == 0u) { const uint32_t h = zse_lit_plain(p, 0u, nlit); wave_copy(p + h, lit, nlit); p += h + nlit; }
    else {
        // weights and codes: the cells of weight w start behind those of the lower weights, 1 << (w - 1) a symbol, the symbols in order
        CJ_LANES(lane) {
            if (lane >= 1u && lane <= 12u) {
                uint32_t c = 0;
                for (uint32_t w = 2; w <= lane; w++) {
                    const uint32_t len = maxlen + 2u - w;                    // the length of weight w - 1
                    c += (len >= 1u && len <= 11u ? D->blc[len] : 0u) << (w - 2u);
                }
                D->blc[16u + lane] = c;
            }
        }
        wave_order();
        CJ_LANES(lane) {
            for (uint32_t s = lane; s < 256u; s += 64u) {
                const uint32_t l = D->lens[s];
                uint32_t v = 0;
                if (l != 0u && l <= maxlen) {
                    const uint32_t w = maxlen + 1u - l;
                    uint32_t idx = 0;
                    for (uint32_t t = 0; t < s; t++) idx += D->lens[t] == l ? 1u : 0u;
                    v = (((D->blc[16u + (w < 12u ? w : 12u)] >> (w - 1u)) + idx) & 0xffffu) | l << 16;
                }
                D->code[s] = v;
            }
        }
        wave_order();
        const uint32_t comp = lsize - lhl, fmt = streams == 1u ? 0u : lhl == 4u ? 2u : 3u, sb = lhl == 3u ? 10u : lhl == 4u ? 14u : 18u;
        zse_bytes(p, 2u | fmt << 2 | (uint64_t)nlit << 4 | (uint64_t)comp << (4u + sb), lhl);
        p += lhl;
        zse_bytes(p, kind == 2u ? wfse : 127u + top, 1u);
        CJ_LANES(lane) {
            if (kind == 2u) {
                for (uint32_t k = lane; k < wfse; k += 64u) out_st8(p + 1u + k, L->wout[k < 224u ? k : 223u]);
            } else {
                const uint32_t s = 2u * lane;
                if (s < top) out_st8(p + 1u + lane, (uint32_t)L->wt[s] << 4 | (s + 1u < top ? L->wt[s + 1u] : 0u));
            }
        }
        wave_order();
        p += desc;
        if (streams == 4u) {
            uint64_t jump = 0;
            for (uint32_t q = 0; q < 3u; q++) jump |= (uint64_t)(((lds_ld(&L->acc[4u + q]) + 8u) >> 3) & 0xffffu) << (16u * q);
            zse_bytes(p, jump, 6u);
            p += 6u;
        }
        for (uint32_t q = 0; q < streams; q++) {
            const uint32_t a = q * seg, b = q + 1u == streams ? nlit : a + seg;
            p += zse_huf_stream(L, p, lit, a < nlit ? a : nlit, b < nlit ? b : nlit);
        }
    }
    // the count: one byte below 128, two below 0x7F00 — a piece of 64 KiB holds at most 16 384 matches of four bytes, so the three-byte
    // form is never needed
    if (nseq < 128u) { zse_bytes(p, nseq, 1u); p += 1u; }
    else { zse_bytes(p, ((nseq >> 8) + 0x80u) | (nseq & 0xffu) << 8, 2u); p += 2u; }
    if (nseq != 0u) {
        zse_bytes(p, tmode[0] << 6 | tmode[1] << 4 | tmode[2] << 2, 1u);
        p += 1u;
        for (uint32_t t = 0; t < 3u; t++) {                              // the descriptions: an RLE table's code, an FSE_Compressed table's NCount
            if (tmode[t] == 1u) zse_bytes(p, rle_sym[t], 1u);
            if (tmode[t] == 2u) {
                CJ_LANES(lane) { for (uint32_t k = lane; k < tncb[t]; k += 64u) out_st8(p + k, L->nc[t][k < 96u ? k : 95u]); }
                wave_order();
            }
            p += tncb[t];
        }
        // pass B: two lanes a sequence, the last sequence first
        DfeOut W;
        dfe_out_init(D, W, p, 0u);
        for (uint32_t done = 0; done < nseq; done += 32u) {
            const uint32_t hi = nseq - done, cnt = hi < 32u ? hi : 32u;
            LaneU64 val;
            LaneU32 nb;
            CJ_LANES(lane) {
                nb[lane] = 0u; val[lane] = 0ull;
                if ((lane >> 1) < cnt) {
                    const uint32_t i = hi - 1u - (lane >> 1);
                    const DfeRec q = rec_ld(slot, i);
                    const uint32_t lv = q.lit & 0x1ffffu, dist = q.dist & 0x1ffffu;
                    uint32_t c, bits, base;
                    if ((lane & 1u) == 0u) {
                        const uint32_t rl = q.lit0 >> 17, ro = q.lit >> 17, rm = q.dist >> 17;
                        uint64_t v = ro & 511u;
                        uint32_t n = (ro >> 9) & 15u;
                        v |= (uint64_t)(rm & 511u) << n; n += (rm >> 9) & 15u;
                        v |= (uint64_t)(rl & 511u) << n; n += (rl >> 9) & 15u;
                        zse_ll(lv, c, bits, base);
                        v |= (uint64_t)(lv - base) << n; n += bits;
                        val[lane] = v; nb[lane] = n;
                    } else {
                        const uint32_t before = i != 0u ? rec_ld(slot, i - 1u).dist & 0x1ffffu : prev;
                        zse_ml(q.mlen, c, bits, base);
                        const uint32_t ofv = zse_ofv(lv, dist, before), oc = dfe_ilog2(ofv) & 31u;
                        val[lane] = (uint64_t)(q.mlen - base) | (uint64_t)(ofv - (1u << oc)) << bits;
                        nb[lane] = bits + oc;
                    }
                }
            }
            dfe_put_round(D, W, val, nb);
        }
        if (tlog[2] != 0u) dfe_put(D, W, lds_ld(&L->acc[13]) & ((1u << tlog[2]) - 1u), tlog[2]);
        if (tlog[1] != 0u) dfe_put(D, W, lds_ld(&L->acc[12]) & ((1u << tlog[1]) - 1u), tlog[1]);
        if (tlog[0] != 0u) dfe_put(D, W, lds_ld(&L->acc[11]) & ((1u << tlog[0]) - 1u), tlog[0]);
        dfe_put(D, W, 1u, 1u);
        dfe_flush_bytes(D, W);
        p += W.obyte;
        prev = rec_ld(slot, nseq - 1u).dist & 0x1ffffu;
    }
    O.op += size;
    return true;
}

// ---- the frame --------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t zse_head_bytes(uint64_t n) { return n <= 255u ? 6u : n <= 65536u ? 7u : n <= 65791u ? 8u : 10u; }
// exact worst case of the layout: every piece a Raw block.  <= n + 3 (n / 65536 + 1) + 14
__host__ __device__ inline uint64_t zse_bound(uint64_t n, uint32_t flags) {
    const uint64_t blocks = n == 0u ? 1u : (n + kZsePiece - 1u) / kZsePiece;
    return zse_head_bytes(n) + 3u * blocks + n + ((flags & kZseChecksum) ? 4u : 0u);
}
// magic, Frame_Header_Descriptor, Window_Descriptor above 64 KiB (0x30: 64 KiB, what no match crosses), Frame_Content_Size; false when it does not fit
__device__ __forceinline__ bool zse_begin(ZseOut& O, uint8_t* out, uint32_t cap, uint32_t n, uint32_t flags) {
    O.out = out; O.cap = cap; O.op = 0u;
    const uint32_t h = zse_head_bytes(n), cks = (flags & kZseChecksum) ? 4u : 0u;
    if (h > cap) return false;
    zse_bytes(out, 0xFD2FB528u, 4u);
    uint64_t v;
    if (n <= 255u) v = (0x20u | cks) | (uint64_t)n << 8;
    else if (n <= 65536u) v = (0x60u | cks) | (uint64_t)(n - 256u) << 8;
    else if (n <= 65791u) v = (0x40u | cks) | 0x30u << 8 | (uint64_t)(n - 256u) << 16;
    else v = (0x80u | cks) | 0x30u << 8 | (uint64_t)n << 16;
    zse_bytes(out + 4u, v, h - 4u);
    O.op = h;
    return true;
}
// the content checksum behind the last block (room for it was part of that block's check).  Returns the frame's length
__device__ __forceinline__ uint32_t zse_end(ZseOut& O, uint32_t flags, uint64_t xxh) {
    if (flags & kZseChecksum) { zse_bytes(O.out + O.op, xxh & 0xffffffffull, 4u); O.op += 4u; }
    return O.op;
}

// ---- XXH64 of the input (seed 0): zstd_wave.hpp's zs_xxh64, which reads a decoder's output, restated over the input's accessors ----
constexpr uint64_t kZxP1 = 0x9E3779B185EBCA87ull, kZxP2 = 0xC2B2AE3D27D4EB4Full, kZxP3 = 0x165667B19E3779F9ull, kZxP4 = 0x85EBCA77C2B2AE63ull,
                   kZxP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ uint64_t zse_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
__device__ __forceinline__ uint64_t zse_xx_round(uint64_t acc, uint64_t v) { return zse_rotl(acc + v * kZxP2, 31) * kZxP1; }
// the 32-byte stripes serially, accumulator j on lane j (acc8: eight words of LDS); the tail and the avalanche wave-uniform
__device__ __forceinline__ uint64_t zse_xxh64(uint32_t* acc8, const uint8_t* p, uint32_t n) {
    const uint32_t stripes = n >> 5;
    uint64_t h;
    if (stripes != 0u) {
        CJ_LANES(lane) {
            if (lane < 4u) {
                uint64_t acc = lane == 0u ? kZxP1 + kZxP2 : lane == 1u ? kZxP2 : lane == 2u ? 0ull : 0ull - kZxP1;
                const uint8_t* q = p + 8u * lane;
                for (uint32_t i = 0; i < stripes; i++, q += 32)
                    acc = zse_xx_round(acc, (uint64_t)in_ld32(q) | ((uint64_t)in_ld32(q + 4) << 32));
                acc8[2u * lane] = (uint32_t)acc;
                acc8[2u * lane + 1u] = (uint32_t)(acc >> 32);
            }
        }
        wave_order();
        uint64_t v[4];
        for (uint32_t j = 0; j < 4u; j++) v[j] = (uint64_t)lds_ld(&acc8[2u * j]) | ((uint64_t)lds_ld(&acc8[2u * j + 1u]) << 32);
        h = zse_rotl(v[0], 1) + zse_rotl(v[1], 7) + zse_rotl(v[2], 12) + zse_rotl(v[3], 18);
        for (uint32_t j = 0; j < 4u; j++) h = (h ^ zse_xx_round(0, v[j])) * kZxP1 + kZxP4;
        wave_order();
    } else {
        h = kZxP5;
    }
    h += n;
    uint32_t at = stripes << 5;
    auto le = [&](uint32_t k) { uint64_t x = 0; for (uint32_t j = 0; j < k; j++) x |= (uint64_t)in_ld8(p + at + j) << (8u * j); at += k; return x; };
    while (at + 8u <= n) { h ^= zse_xx_round(0, le(8)); h = zse_rotl(h, 27) * kZxP1 + kZxP4; }
    if (at + 4u <= n) { h ^= le(4) * kZxP1; h = zse_rotl(h, 23) * kZxP2 + kZxP3; }
    while (at < n) { h ^= le(1) * kZxP5; h = zse_rotl(h, 11) * kZxP1; }
    h ^= h >> 33; h *= kZxP2; h ^= h >> 29; h *= kZxP3; h ^= h >> 32;
    return h;
}

}  // namespace cj
