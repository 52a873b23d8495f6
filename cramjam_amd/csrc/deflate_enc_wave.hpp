// deflate_enc_wave.hpp — the entropy stage of the DEFLATE encoder, one wavefront per stream: the sequence records
// that the matcher left in the workgroup's scratch slot become one block per piece — stored, fixed or dynamic by their exact costs —
// behind a bit position that is carried from block to block.  tests/hostsim/deflate_enc_model.c states the same thing as scalar C;
// this text emits exactly its bytes.  Written like deflate_wave.hpp: it names only
//     wave_copy, wave_order, CJ_LANES, LaneU32, LaneU64, lane_excl_add, lds_ld, lds_ld8, lds_add, lds_or, in_ld8, out_st8, out_st32
// of the wave-decoder contract: wave_lanes.hpp + cj_common.hpp implement it for the device,
// tests/hostsim/sim_wave.hpp, with every access bounds-checked, for the host (sim_deflate_encode.cpp), and
//     rec_ld(slot, i)           record i of the scratch slot, which whoever includes this declares (it needs the complete DfeRec)
// Not part of the C-ABI.
//
// Mapping.  The bit position, the block's costs and its choice are wave-uniform.  The lanes take CONSECUTIVE SYMBOLS: 64 records are
// loaded, a prefix sum over their symbol counts (literals + split matches) gives every symbol its record, and a round is 64 symbols —
// counted into the histograms in the first pass, coded in the second (at most 48 bits a symbol: 15 + 5 + 15 + 13).  A prefix sum over
// the bit lengths gives every lane its bit offset, the bits are OR-ed into a staging area in LDS, whole dwords leave with vector
// stores and the bits behind the last whole dword stay for the next round and the next block.  The code lengths are built by rank
// (every lane counts the symbols below its own: a sort without a loop over the lanes) and one lane's two-queue Huffman walk over at
// most 286 sorted counts; the repair of an over-long code works on the sixteen per-length counts alone.
// Every loop is bounded by the piece's length or an alphabet's size; every index into LDS or the slot is masked or compared.
#pragma once
#include <stdint.h>

namespace cj {

constexpr uint32_t kDfePiece = 65536u;                // bytes of a piece: the lap of the matcher's 16-bit table
constexpr uint32_t kDfeSlotRecs = kDfePiece / 4u + 2u;   // records of a scratch slot: a sequence covers at least four bytes, + the final literals
constexpr uint32_t kDfeInMax = 0x7E000000u;

struct DfeRec { uint32_t lit0, lit, dist, mlen; };    // literals [lit0, lit0 + lit) of the piece, then mlen bytes from dist back (mlen 0: none)

// The wavefront's LDS: 11.3 KiB
struct DfeLds {
    uint32_t hist[320];      // symbol counts: literal/length at 0, distance at 288
    uint32_t code[320];      // bit-reversed code | length << 16, the same places
    uint32_t cl_hist[32], cl_code[32];
    uint32_t key[288];       // code builder: count << 9 | symbol (unused: ~0)
    uint32_t sw[288], iw[288];     // sorted leaf weights, internal node weights
    uint32_t blc[32];        // codes per length; first code per length at 16
    uint32_t stage[128];     // the bit writer's staging area; stage[0] holds the bits carried over
    uint32_t pre[64];        // first symbol of each of the round's records
    DfeRec rl[64];
    uint32_t acc[8];         // 0 used symbols, 1 tokens, 2 / 3 dynamic / fixed cost
    uint16_t par[576];       // parent of leaf i / of internal node k at 288 + k
    uint16_t rk[288];        // rank of a symbol among the used ones
    uint16_t tok[320];       // the run-length coded code lengths: symbol | extra value << 8
    uint8_t lens[320], cl_lens[32];
    uint8_t idep[288];       // depth of an internal node
};

// the output of one stream: stage[0]'s low `c` bits are pending and belong at byte `obyte`
struct DfeOut { uint8_t* out; uint32_t cap, obyte, c; };

__device__ __forceinline__ uint32_t dfe_ilog2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v | 1u); }
__device__ __forceinline__ uint32_t dfe_bitrev(uint32_t v, uint32_t n) {      // the low n bits of v, reversed (1 <= n <= 15)
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32u - n);
}
__device__ __forceinline__ uint32_t dfe_n_split(uint32_t m) { return m ? (m + 257u) / 258u : 0u; }
// piece j of k of a match of m bytes: 258 each, the last two arranged so that none is below 3 (259 = 256 + 3)
__device__ __forceinline__ uint32_t dfe_split_len(uint32_t m, uint32_t k, uint32_t j) {
    const uint32_t rem = m - 258u * (k - 1u);
    if (j + 1u == k) return rem < 3u ? 3u : rem;
    if (j + 2u == k && rem < 3u) return 258u - (3u - rem);
    return 258u;
}
__device__ __forceinline__ void dfe_len_sym(uint32_t L, uint32_t& sym, uint32_t& xb, uint32_t& xv) {      // 3 <= L <= 258
    const uint32_t l = L - 3u;
    sym = 285u; xb = 0u; xv = 0u;
    if (L >= 258u) return;
    if (l < 8u) { sym = 257u + l; return; }
    const uint32_t e = dfe_ilog2(l) - 2u;
    sym = 261u + 4u * e + ((l >> e) & 3u); xb = e; xv = l & ((1u << e) - 1u);
}
__device__ __forceinline__ void dfe_dist_sym(uint32_t D, uint32_t& sym, uint32_t& xb, uint32_t& xv) {     // 1 <= D <= 32768
    const uint32_t dd = D - 1u;
    sym = dd; xb = 0u; xv = 0u;
    if (dd < 4u) return;
    const uint32_t hb = dfe_ilog2(dd), e = hb - 1u;
    sym = 2u * hb + ((dd >> e) & 1u); xb = e; xv = dd & ((1u << e) - 1u);
}
__device__ __forceinline__ uint32_t dfe_len_xb(uint32_t s) { return s < 265u || s >= 285u ? 0u : (s - 261u) / 4u; }
__device__ __forceinline__ uint32_t dfe_dist_xb(uint32_t s) { return s < 4u ? 0u : (s >> 1) - 1u; }
__device__ __forceinline__ uint32_t dfe_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
__device__ __forceinline__ uint32_t dfe_tok_xb(uint32_t s) { return s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u; }
__device__ __forceinline__ uint32_t dfe_cl_order(uint32_t k) {      // the order of the code-length code's lengths, five bits each
    constexpr uint64_t w0 = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t w1 = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12u ? w0 >> (5u * k) : w1 >> (5u * ((k - 12u) & 7u))) & 31u);
}

// ---- the bit writer ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dfe_out_init(DfeLds* L, DfeOut& W, uint8_t* out, uint32_t cap) {
    W.out = out; W.cap = cap; W.obyte = 0u; W.c = 0u;
    CJ_LANES(lane) { L->stage[lane] = 0u; L->stage[64u + lane] = 0u; }
    wave_order();
}
__device__ __forceinline__ uint64_t dfe_bitpos(const DfeOut& W) { return 8ull * W.obyte + W.c; }
// n <= 32 bits, wave-uniform
__device__ __forceinline__ void dfe_put(DfeLds* L, DfeOut& W, uint32_t v, uint32_t n) {
    const uint64_t x = (uint64_t)v << W.c;
    CJ_LANES(lane) { if (lane == 0u) { L->stage[0] |= (uint32_t)x; L->stage[1] = (uint32_t)(x >> 32); } }
    wave_order();
    W.c += n;
    if (W.c >= 32u) {
        CJ_LANES(lane) { if (lane == 0u) { out_st32(W.out + W.obyte, L->stage[0]); L->stage[0] = L->stage[1]; } }
        W.obyte += 4u; W.c -= 32u;
    }
    CJ_LANES(lane) { if (lane == 0u) L->stage[1] = 0u; }
    wave_order();
}
// the pending bits out as whole bytes (zero bits fill the last one)
__device__ __forceinline__ void dfe_flush_bytes(DfeLds* L, DfeOut& W) {
    const uint32_t nb = (W.c + 7u) >> 3;
    CJ_LANES(lane) { if (lane < nb) out_st8(W.out + W.obyte + lane, (L->stage[0] >> (8u * lane)) & 0xffu); }
    wave_order();
    CJ_LANES(lane) { if (lane == 0u) L->stage[0] = 0u; }
    wave_order();
    W.obyte += nb; W.c = 0u;
}
// one round: lane's nb[lane] <= 48 bits of val[lane], in lane order
__device__ __forceinline__ void dfe_put_round(DfeLds* L, DfeOut& W, LaneU64& val, LaneU32& nb) {
    LaneU32 before;
    const uint32_t total = lane_excl_add(nb, before);
    CJ_LANES(lane) {
        if (nb[lane] != 0u) {
            const uint32_t bit = W.c + before[lane], w = bit >> 5, sh = bit & 31u;
            const uint64_t v = val[lane], x = v << sh;
            const uint32_t d0 = (uint32_t)x, d1 = (uint32_t)(x >> 32), d2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
            if (d0) lds_or(&L->stage[w & 127u], d0);
            if (d1) lds_or(&L->stage[(w + 1u) & 127u], d1);
            if (d2) lds_or(&L->stage[(w + 2u) & 127u], d2);
        }
    }
    wave_order();
    const uint32_t T = W.c + total, D = T >> 5;              // (T <= 31 + 64 * 48: D <= 96)
    CJ_LANES(lane) {
        for (uint32_t k = lane; k < D; k += 64u) out_st32(W.out + W.obyte + 4u * k, L->stage[k & 127u]);
    }
    wave_order();
    const uint32_t carry = lds_ld(&L->stage[D & 127u]);
    wave_order();
    CJ_LANES(lane) { L->stage[lane] = lane == 0u ? carry : 0u; L->stage[64u + lane] = 0u; }
    wave_order();
    W.obyte += 4u * D; W.c = T & 31u;
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------
// Length-limited code lengths of hist[0, nsym) into lens[0, nsym), nsym <= 288, maxbits <= 15: Huffman over the used symbols in
// (count, symbol) order, depths above maxbits folded into it, the Kraft sum repaired one unit at a time, the lengths dealt out by rank.
// One used symbol gets length 1 (pad_single: and a second symbol beside it, for the alphabet whose code inflate wants complete).
__device__ __forceinline__ void dfe_build_lens(DfeLds* L, const uint32_t* hist, uint32_t nsym, uint32_t maxbits, bool pad_single, uint8_t* lens) {
    CJ_LANES(lane) {
        if (lane == 0u) L->acc[0] = 0u;
        for (uint32_t s = lane; s < nsym; s += 64u) { L->key[s] = hist[s] ? (hist[s] << 9) | s : ~0u; lens[s] = 0u; }
    }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) {
            const uint32_t mine = L->key[s];
            if (mine == ~0u) continue;
            uint32_t r = 0;
            for (uint32_t t = 0; t < nsym; t++) r += L->key[t] < mine ? 1u : 0u;
            L->rk[s] = (uint16_t)r;
            L->sw[r] = mine >> 9;
            lds_add(&L->acc[0], 1u);
        }
    }
    wave_order();
    const uint32_t n = lds_ld(&L->acc[0]);
    if (n == 0u) return;
    if (n == 1u) {
        CJ_LANES(lane) {
            for (uint32_t s = lane; s < nsym; s += 64u) {
                if (L->key[s] != ~0u) { lens[s] = 1u; if (pad_single) lens[s == 0u ? 1u : 0u] = 1u; }
            }
        }
        wave_order();
        return;
    }
    CJ_LANES(lane) {
        if (lane == 0u) {
            uint32_t li = 0, ii = 0;
            for (uint32_t ni = 0; ni + 1u < n; ni++) {                 // the two queues: sorted leaves, internal nodes in the order they were made
                uint32_t w = 0;
                for (int pick = 0; pick < 2; pick++) {
                    if (li < n && (ii >= ni || L->sw[li] <= L->iw[ii])) { w += L->sw[li]; L->par[li] = (uint16_t)ni; li++; }
                    else { w += L->iw[ii]; L->par[288u + ii] = (uint16_t)ni; ii++; }
                }
                L->iw[ni] = w;
            }
            L->idep[n - 2u] = 0u;
            for (uint32_t k = n - 2u; k-- > 0u;) {
                const uint32_t up = L->idep[L->par[288u + k] % 288u] + 1u;
                L->idep[k] = (uint8_t)(up < 255u ? up : 255u);
            }
            for (uint32_t l = 0; l < 32u; l++) L->blc[l] = 0u;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t d = L->idep[L->par[i] % 288u] + 1u;
                L->blc[d < maxbits ? d : maxbits] += 1u;
            }
            uint32_t total = 0;
            for (uint32_t l = 1; l <= maxbits; l++) total += L->blc[l] << (maxbits - l);
            while (total > (1u << maxbits)) {                          // (every turn takes one unit: fewer turns than symbols)
                L->blc[maxbits] -= 1u;
                for (uint32_t l = maxbits - 1u; l > 0u; l--)
                    if (L->blc[l] != 0u) { L->blc[l] -= 1u; L->blc[l + 1u] += 2u; break; }
                total -= 1u;
            }
        }
    }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) {
            if (L->key[s] == ~0u) continue;
            const uint32_t r = L->rk[s];
            uint32_t c = 0, len = 1;
            for (uint32_t l = maxbits; l >= 1u; l--) { c += L->blc[l]; if (r < c) { len = l; break; } }
            lens[s] = (uint8_t)len;
        }
    }
    wave_order();
}

// canonical codes (RFC 1951 3.2.2) of lens[0, nsym), bit-reversed, with their lengths: code[s] = reversed | length << 16
__device__ __forceinline__ void dfe_assign_codes(DfeLds* L, const uint8_t* lens, uint32_t nsym, uint32_t maxbits, uint32_t* code) {
    CJ_LANES(lane) { if (lane < 32u) L->blc[lane] = 0u; }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) if (lens[s] != 0u) lds_add(&L->blc[lens[s] & 15u], 1u);
    }
    wave_order();
    CJ_LANES(lane) {
        if (lane >= 1u && lane <= maxbits) {
            uint32_t c = 0;
            for (uint32_t l = 1; l <= lane; l++) c = (c + (l > 1u ? L->blc[l - 1u] : 0u)) << 1;
            L->blc[16u + lane] = c;
        }
    }
    wave_order();
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < nsym; s += 64u) {
            const uint32_t l = lens[s] & 15u;
            uint32_t v = 0;
            if (l != 0u) {
                uint32_t idx = 0;
                for (uint32_t t = 0; t < s; t++) idx += lens[t] == l ? 1u : 0u;
                v = dfe_bitrev(L->blc[16u + l] + idx, l) | (l << 16);
            }
            code[s] = v;
        }
    }
    wave_order();
}

// ---- the symbols of a piece ---------------------------------------------------------------------------------------------------------
// WRITE false: count them into L->hist; true: code them with L->code.  slot: the piece's nrec records; in: its pn bytes
template <bool WRITE>
__device__ __forceinline__ void dfe_symbols(DfeLds* L, DfeOut& W, const uint8_t* in, uint32_t pn, const DfeRec* slot, uint32_t nrec) {
    for (uint32_t r0 = 0; r0 < nrec; r0 += 64u) {
        LaneU32 ns, before;
        CJ_LANES(lane) {
            DfeRec q = {0u, 0u, 1u, 0u};
            if (r0 + lane < nrec) q = rec_ld(slot, r0 + lane);
            // what the matcher wrote lies inside the piece; nothing below relies on that
            if (q.lit0 > pn) q.lit0 = pn;
            if (q.lit > pn - q.lit0) q.lit = pn - q.lit0;
            if (q.mlen > kDfePiece || q.mlen < 3u || q.dist == 0u || q.dist > 32768u) q.mlen = 0u;
            L->rl[lane] = q;
            ns[lane] = q.lit + dfe_n_split(q.mlen);
        }
        const uint32_t total = lane_excl_add(ns, before);
        CJ_LANES(lane) { L->pre[lane] = before[lane]; }
        wave_order();
        for (uint32_t s0 = 0; s0 < total; s0 += 64u) {
            LaneU64 val;
            LaneU32 nb;
            CJ_LANES(lane) {
                const uint32_t k = s0 + lane;
                nb[lane] = 0u; val[lane] = 0ull;
                if (k < total) {
                    uint32_t r = 0;                                       // the last record that starts at or before symbol k
                    for (uint32_t step = 32u; step != 0u; step >>= 1) if (L->pre[(r + step) & 63u] <= k) r += step;
                    const DfeRec q = L->rl[r & 63u];
                    const uint32_t j = k - L->pre[r & 63u];
                    uint32_t sym, xb = 0, xv = 0, dsym = 0, dxb = 0, dxv = 0;
                    const bool lit = j < q.lit;
                    if (lit) sym = in_ld8(in + q.lit0 + j);
                    else {
                        const uint32_t kk = dfe_n_split(q.mlen), jj = j - q.lit;
                        dfe_len_sym(dfe_split_len(q.mlen, kk, jj < kk ? jj : kk - 1u), sym, xb, xv);
                        dfe_dist_sym(q.dist, dsym, dxb, dxv);
                    }
                    if (!WRITE) {
                        lds_add(&L->hist[sym], 1u);
                        if (!lit) lds_add(&L->hist[288u + dsym], 1u);
                    } else {
                        const uint32_t c = L->code[sym], cl = c >> 16;
                        uint64_t v = (c & 0xffffu) | ((uint64_t)xv << cl);
                        uint32_t n = cl + xb;
                        if (!lit) {
                            const uint32_t d = L->code[288u + dsym], dl = d >> 16;
                            v |= (uint64_t)((d & 0xffffu) | (dxv << dl)) << n;
                            n += dl + dxb;
                        }
                        val[lane] = v; nb[lane] = n;
                    }
                }
            }
            if (WRITE) dfe_put_round(L, W, val, nb);
        }
        wave_order();
    }
}

__device__ __forceinline__ void dfe_put_stored(DfeLds* L, DfeOut& W, const uint8_t* p, uint32_t len, bool final) {
    dfe_put(L, W, final ? 1u : 0u, 3u);
    dfe_flush_bytes(L, W);
    dfe_put(L, W, len | ((len ^ 0xffffu) << 16), 32u);
    wave_copy(W.out + W.obyte, p, len);
    W.obyte += len;
}

// One piece (pn <= 65536 bytes at in, its nrec records at slot) as one block behind W's bit position; `final` sets BFINAL.  tail: bytes
// the stream still needs behind its last block (the final pad is counted here).  Returns false, before the block's first store, when
// the block (and, for the final one, the tail) does not fit the capacity.  type (may be null): 0 stored, 1 fixed, 2 dynamic
__device__ __forceinline__ bool dfe_piece(DfeLds* L, DfeOut& W, const uint8_t* in, uint32_t pn, const DfeRec* slot, uint32_t nrec, bool final,
                                          uint32_t tail, uint32_t* type) {
    CJ_LANES(lane) {
        for (uint32_t s = lane; s < 320u; s += 64u) { L->hist[s] = 0u; L->lens[s] = 0u; }      // (symbols 286 / 287 and 30 / 31 keep length 0)
        if (lane < 32u) { L->cl_hist[lane] = 0u; L->cl_lens[lane] = 0u; }
        if (lane < 8u) L->acc[lane] = 0u;
    }
    wave_order();
    dfe_symbols<false>(L, W, in, pn, slot, nrec);
    CJ_LANES(lane) { if (lane == 0u) L->hist[256] += 1u; }
    wave_order();
    dfe_build_lens(L, L->hist, 286u, 15u, false, L->lens);
    dfe_build_lens(L, L->hist + 288u, 30u, 15u, false, L->lens + 288u);
    // HLIT, HDIST; the two alphabets' lengths as one run-length coded sequence (one lane: at most 316 lengths)
    uint32_t hlit = 286u, hdist = 30u;
    while (hlit > 257u && lds_ld8(&L->lens[hlit - 1u]) == 0u) hlit--;
    while (hdist > 1u && lds_ld8(&L->lens[288u + hdist - 1u]) == 0u) hdist--;
    CJ_LANES(lane) {
        if (lane == 0u) {
            const uint32_t m = hlit + hdist;
            uint32_t nt = 0, i = 0;
            while (i < m) {
                const uint32_t v = L->lens[i < hlit ? i : 288u + (i - hlit)];
                uint32_t run = 1;
                while (i + run < m && L->lens[i + run < hlit ? i + run : 288u + (i + run - hlit)] == v) run++;
                i += run;
                if (v == 0u) {
                    while (run >= 11u) { const uint32_t r = run < 138u ? run : 138u; L->tok[nt++ % 320u] = (uint16_t)(18u | (r - 11u) << 8); run -= r; }
                    if (run >= 3u) { L->tok[nt++ % 320u] = (uint16_t)(17u | (run - 3u) << 8); run = 0u; }
                    while (run != 0u) { L->tok[nt++ % 320u] = 0u; run--; }
                } else {
                    L->tok[nt++ % 320u] = (uint16_t)v; run--;
                    while (run >= 3u) { const uint32_t r = run < 6u ? run : 6u; L->tok[nt++ % 320u] = (uint16_t)(16u | (r - 3u) << 8); run -= r; }
                    while (run != 0u) { L->tok[nt++ % 320u] = (uint16_t)v; run--; }
                }
            }
            L->acc[1] = nt;
        }
    }
    wave_order();
    const uint32_t nt = lds_ld(&L->acc[1]) < 320u ? lds_ld(&L->acc[1]) : 320u;
    CJ_LANES(lane) {
        for (uint32_t i = lane; i < nt; i += 64u) lds_add(&L->cl_hist[L->tok[i] & 31u], 1u);
    }
    wave_order();
    dfe_build_lens(L, L->cl_hist, 19u, 7u, true, L->cl_lens);
    uint32_t hclen = 19u;
    while (hclen > 4u && lds_ld8(&L->cl_lens[dfe_cl_order(hclen - 1u)]) == 0u) hclen--;
    // the exact costs
    CJ_LANES(lane) {
        uint32_t dyn = 0, fix = 0;
        for (uint32_t i = lane; i < nt; i += 64u) { const uint32_t s = L->tok[i] & 31u; dyn += L->cl_lens[s] + dfe_tok_xb(s); }
        for (uint32_t s = lane; s < 286u; s += 64u) { const uint32_t h = L->hist[s], x = dfe_len_xb(s); dyn += h * (L->lens[s] + x); fix += h * (dfe_fixed_len(s) + x); }
        if (lane < 30u) { const uint32_t h = L->hist[288u + lane], x = dfe_dist_xb(lane); dyn += h * (L->lens[288u + lane] + x); fix += h * (5u + x); }
        lds_add(&L->acc[2], dyn);
        lds_add(&L->acc[3], fix);
    }
    wave_order();
    const uint64_t at = dfe_bitpos(W);
    const uint64_t dyn = 3u + 14u + 3u * hclen + (uint64_t)lds_ld(&L->acc[2]), fix = 3u + (uint64_t)lds_ld(&L->acc[3]);
    const uint32_t pad = (8u - (uint32_t)((at + 3u) & 7u)) & 7u;
    uint64_t sto = 3u + pad + 32u + 8ull * pn;
    if (pn == kDfePiece) sto += 3u + 5u + 32u;
    const uint32_t t = (sto <= fix && sto <= dyn) ? 0u : fix <= dyn ? 1u : 2u;
    if (type) *type = t;
    const uint64_t cost = t == 0u ? sto : t == 1u ? fix : dyn;
    if (((at + cost + 7u) >> 3) + (final ? tail : 0u) > W.cap) return false;
    if (t == 0u) {
        if (pn == kDfePiece) { dfe_put_stored(L, W, in, 65535u, false); dfe_put_stored(L, W, in + 65535u, 1u, final); }
        else dfe_put_stored(L, W, in, pn, final);
        return true;
    }
    if (t == 1u) {
        CJ_LANES(lane) {
            for (uint32_t s = lane; s < 320u; s += 64u) L->lens[s] = (uint8_t)(s < 288u ? dfe_fixed_len(s) : 5u);
        }
        wave_order();
    }
    dfe_assign_codes(L, L->lens, 288u, 15u, L->code);
    dfe_assign_codes(L, L->lens + 288u, 32u, 15u, L->code + 288u);
    dfe_put(L, W, (final ? 1u : 0u) | (t << 1), 3u);
    if (t == 2u) {
        dfe_assign_codes(L, L->cl_lens, 19u, 7u, L->cl_code);
        dfe_put(L, W, (hlit - 257u) | ((hdist - 1u) << 5) | ((hclen - 4u) << 10), 14u);
        // the header's items through the lanes: the code-length code's lengths, then the tokens
        const uint32_t items = hclen + nt;
        for (uint32_t i0 = 0; i0 < items; i0 += 64u) {
            LaneU64 val;
            LaneU32 nb;
            CJ_LANES(lane) {
                const uint32_t i = i0 + lane;
                nb[lane] = 0u; val[lane] = 0ull;
                if (i < hclen) { val[lane] = L->cl_lens[dfe_cl_order(i)]; nb[lane] = 3u; }
                else if (i < items) {
                    const uint32_t tk = L->tok[(i - hclen) % 320u], s = tk & 31u, c = L->cl_code[s], cl = c >> 16;
                    val[lane] = (c & 0xffffu) | ((uint64_t)(tk >> 8) << cl);
                    nb[lane] = cl + dfe_tok_xb(s);
                }
            }
            dfe_put_round(L, W, val, nb);
        }
    }
    dfe_symbols<true>(L, W, in, pn, slot, nrec);
    const uint32_t eob = lds_ld(&L->code[256]);
    dfe_put(L, W, eob & 0xffffu, eob >> 16);
    return true;
}

constexpr int kDfeRaw = 0, kDfeZlib = 1, kDfeGzip = 2;      // cj_deflate_wrap (the one set of names: the decoder compares with the C-ABI's enum)
__device__ __forceinline__ uint32_t dfe_head_bytes(int wrap) { return wrap == kDfeZlib ? 2u : wrap == kDfeGzip ? 10u : 0u; }
__device__ __forceinline__ uint32_t dfe_tail_bytes(int wrap) { return wrap == kDfeZlib ? 4u : wrap == kDfeGzip ? 8u : 0u; }

// the wrapper's header; false when it does not fit
__device__ __forceinline__ bool dfe_begin(DfeLds* L, DfeOut& W, int wrap, uint8_t* out, uint32_t cap) {
    dfe_out_init(L, W, out, cap);
    if (dfe_head_bytes(wrap) > cap) return false;
    if (wrap == kDfeZlib) dfe_put(L, W, 0x0178u, 16u);                       // CM 8, CINFO 7; FLG 01: no dictionary, FCHECK
    if (wrap == kDfeGzip) { dfe_put(L, W, 0x00088b1fu, 32u); dfe_put(L, W, 0u, 32u); dfe_put(L, W, 0xff00u, 16u); }      // no flags, MTIME 0, XFL 0, OS 255
    return true;
}
// the last byte's unused bits (0), then the trailer: sum = Adler-32 / CRC-32 of the n input bytes.  Returns the stream's length
__device__ __forceinline__ uint32_t dfe_end(DfeLds* L, DfeOut& W, int wrap, uint32_t sum, uint32_t n) {
    dfe_flush_bytes(L, W);
    if (wrap == kDfeZlib) dfe_put(L, W, __builtin_bswap32(sum), 32u);
    if (wrap == kDfeGzip) { dfe_put(L, W, sum, 32u); dfe_put(L, W, n, 32u); }
    return W.obyte;
}

// exact worst case of the layout: every piece stored (two blocks for a full one), each behind a header that may spill into a new byte
__host__ __device__ inline uint64_t dfe_bound(uint64_t n, int wrap) {
    const uint64_t full = n / kDfePiece, rest = (n % kDfePiece != 0u || n == 0u) ? 1u : 0u;
    return n + 10u * full + 5u * rest + (wrap == kDfeZlib ? 6u : wrap == kDfeGzip ? 18u : 0u);
}

}  // namespace cj
