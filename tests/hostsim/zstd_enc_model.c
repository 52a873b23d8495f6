/* zstd_enc_model.c — scalar CPU statement of the Zstandard encoder of cramjam_amd/csrc/zstd_encode.hip (TEST INFRASTRUCTURE;
 * DESIGN.md 5.15).  The kernel and the host build of its entropy stage (sim_zstd_encode.cpp) emit exactly these bytes.
 *
 *   frame     magic, descriptor, Frame_Content_Size always: n <= 65536 Single_Segment with 1 (n <= 255) or 2 bytes; above that a
 *             Window_Descriptor of 0x30 (64 KiB: no match crosses a piece) and 2 (n <= 65791) or 4 bytes.  No dictionary id
 *   pieces    the input is cut into independent pieces of at most 65 536 bytes, one block each: RLE (one repeated byte), Compressed
 *             (its exact size is below the piece's) or Raw.  An empty input is a header and one empty last Raw block
 *   matching  enc2_round.h's round (no distance limit but the 16-bit table's lap), R = 512, last_start =
 *             n - 8, limit = n; a piece below 8 bytes is all literals.  Records (literal start, literal count, distance, match length)
 *   literals  all literal runs in order: Raw or Huffman by exact size (one distinct literal is one distinct byte: an RLE block), a tie to the simpler.  Huffman: the
 *             DEFLATE model's builder at limit 11 (dfe_model_build_lens, linked in), weight = max length + 1 - length, codes by
 *             (weight, symbol) as libzstd's decoder lays its table; the tree as direct 4-bit weights (at most 128 of them) or FSE-compressed
 *             weights, whichever is smaller; one stream up to 1023 literals, four above; sizes in the 10 / 14 / 18-bit header forms
 *   sequences count in 1 or 2 bytes; LL / OF / ML each RLE (one code used), FSE_Compressed or Predefined by an estimated cost (zstd_fse_enc.h); offsets distance + 3, or the repeat code 1
 *             when the literal length is > 0 and the distance is that of the frame's previous sequence (initially 1); the backward
 *             bitstream in libzstd's order with the final 1-bit
 *   checksum  the low 32 bits of XXH64 (seed 0) of the input, behind the last block, when asked for
 */
#include "enc2_round.h"
#include "../../cramjam_amd/csrc/zstd_fse_enc.h"      /* the FSE stage's serial arithmetic: the kernel includes the same text */

#define ZPIECE 65536u
#define ZE_OUT_TOO_SMALL (-6)
#define ZE_INPUT_TOO_LARGE (-1)
#define ZIN_MAX 0x7E000000u

uint32_t dfe_model_build_lens(const uint32_t* hist, uint32_t nsym, uint32_t maxbits, int pad_single, uint8_t* lens);

typedef enc2_rec_t zrec_t;

/* the records of one piece (n <= 65536); rec must hold n / 4 + 2 records.  Returns their number (the last one has no match) */
uint32_t zse_model_records(const uint8_t* in, uint32_t n, uint32_t* rec_out) { return enc2_records(in, n, ENC2_NO_MAX_DIST, 512u, rec_out); }

/* ---- the codes ------------------------------------------------------------------------------------------------------------------- */
static const uint32_t kLLBase[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024,
                                     2048, 4096, 8192, 16384, 32768, 65536};
static const uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
static const uint32_t kMLBase[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                                     35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
static const uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                    1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
static const int8_t kLLNorm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
static const int8_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
static const int8_t kMLNorm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};

static uint32_t hb(uint32_t v) { uint32_t r = 0; while (v >>= 1) r++; return r; }
static uint32_t code_of(uint32_t v, const uint32_t* base, uint32_t n) { uint32_t c = 0; for (uint32_t k = 1; k < n; k++) if (base[k] <= v) c = k; return c; }

/* ---- FSE: the encoder's tables from normalized counts (-1: a "less than one" symbol), as libzstd's decoder expects them ------------- */
typedef struct { uint16_t st[512]; uint32_t dnb[64]; int32_t dfs[64]; uint32_t log; int rle; } ctab_t;

static void fse_ctab(ctab_t* t, const int16_t* norm, uint32_t nsym, uint32_t log) {
    uint8_t cell[512];
    uint32_t cumul[64];
    t->log = log; t->rle = 0;
    zsf_table(norm, nsym, log, t->st, t->dnb, t->dfs, cell, cumul);
}

/* ---- the bit writer (libzstd's BIT_CStream: bits at rising positions, read back from the end) ---------------------------------------- */
typedef struct { uint8_t* out; uint64_t pos; uint64_t acc; uint32_t cnt; } bw_t;
static void put(bw_t* w, uint32_t v, uint32_t n) {
    if (n == 0) return;
    w->acc |= (uint64_t)(v & (n >= 32u ? 0xffffffffu : (1u << n) - 1u)) << w->cnt;
    w->cnt += n;
    while (w->cnt >= 8u) { w->out[w->pos++] = (uint8_t)w->acc; w->acc >>= 8; w->cnt -= 8u; }
}
static uint32_t close_stream(bw_t* w) {            /* the final 1-bit, zeros up to the byte; returns the bits of the last byte before it */
    const uint32_t at = w->cnt;
    put(w, 1, 1);
    if (w->cnt) { w->out[w->pos++] = (uint8_t)w->acc; w->acc = 0; w->cnt = 0; }
    return at;
}

typedef struct { uint32_t state; const ctab_t* t; } cst_t;
static void st_init(cst_t* c, const ctab_t* t, uint32_t sym) {
    c->t = t;
    if (t->rle) { c->state = 0; return; }
    const uint32_t nb = (t->dnb[sym] + (1u << 15)) >> 16, v = (nb << 16) - t->dnb[sym];
    c->state = t->st[(int32_t)(v >> nb) + t->dfs[sym]];
}
static void st_put(bw_t* w, cst_t* c, uint32_t sym) {
    if (c->t->rle) return;
    const uint32_t nb = (c->state + c->t->dnb[sym]) >> 16;
    put(w, c->state, nb);
    c->state = c->t->st[(int32_t)(c->state >> nb) + c->t->dfs[sym]];
}
static void st_flush(bw_t* w, const cst_t* c) { if (!c->t->rle) put(w, c->state, c->t->log); }

/* ---- literals ------------------------------------------------------------------------------------------------------------------------ */
enum { LIT_RAW = 0, LIT_RLE = 1, LIT_HUF = 2 };
static uint32_t lit_hdr_plain(uint8_t* o, uint32_t type, uint32_t n) {
    if (n <= 31u) { if (o) o[0] = (uint8_t)(type | n << 3); return 1; }
    if (n <= 4095u) { if (o) { const uint32_t v = type | 1u << 2 | n << 4; o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); } return 2; }
    if (o) { const uint32_t v = type | 3u << 2 | n << 4; o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); }
    return 3;
}
static uint32_t lit_hdr_huf_len(uint32_t n) { return n <= 1023u ? 3u : n <= 16383u ? 4u : 5u; }

/* One piece's literals section into o (room for n + 8 bytes).  Returns its length; info[0] mode, info[1] streams, info[2] tree kind (1 direct weights, 2 FSE-compressed weights) */
static uint32_t put_literals(uint8_t* o, const uint8_t* lit, uint32_t n, uint32_t* info) {
    uint32_t hist[256] = {0}, used = 0, top = 0;
    for (uint32_t i = 0; i < n; i++) hist[lit[i]]++;
    for (uint32_t s = 0; s < 256u; s++) if (hist[s]) { used++; top = s; }
    const uint32_t raw = lit_hdr_plain(0, 0, n) + n;
    uint32_t best = raw, mode = LIT_RAW;
    uint8_t lens[256];
    uint32_t code[256], maxlen = 0, streams = n <= 1023u ? 1u : 4u, seg = (n + 3u) / 4u, sbytes[4] = {0, 0, 0, 0}, desc = 0;
    uint8_t wt[256], wout[224];
    uint32_t kind = 0, deepest = 0, fse = 0;
    if (used >= 2u) {
        deepest = dfe_model_build_lens(hist, 256, 11, 0, lens);
        for (uint32_t s = 0; s < 256u; s++) if (lens[s] > maxlen) maxlen = lens[s];
        for (uint32_t s = 0; s < 256u; s++) wt[s] = lens[s] ? (uint8_t)(maxlen + 1u - lens[s]) : 0u;
        /* the tree: direct 4-bit weights (at most 128 of them) or FSE-compressed weights, whichever is smaller; a tie to the direct ones */
        uint32_t wh[16], wd[64], wc[64];
        int32_t wf[64];
        int16_t wn[16];
        uint16_t ws[64];
        uint8_t cell[64];
        fse = zsf_weights(wt, top, wout, sizeof wout, wh, wn, ws, wd, wf, cell, wc);
        if (top <= 128u) { desc = 1u + (top + 1u) / 2u; kind = 1; }
        if (fse != 0u && (kind == 0u || 1u + fse < desc)) { desc = 1u + fse; kind = 2; }
    }
    if (kind != 0u) {
        uint32_t total = lit_hdr_huf_len(n) + desc + (streams == 4u ? 6u : 0u);
        for (uint32_t q = 0; q < streams; q++) {
            const uint32_t a = streams == 1u ? 0u : q * seg, b = streams == 1u ? n : (q == 3u ? n : a + seg);
            uint64_t bits = 1;
            for (uint32_t i = a; i < b; i++) bits += lens[lit[i]];
            sbytes[q] = (uint32_t)((bits + 7u) >> 3);
            total += sbytes[q];
        }
        if (total < best) { best = total; mode = LIT_HUF; info[10] = deepest; info[11] = used; }
    }
    info[0] = mode; info[1] = mode == LIT_HUF ? streams : 0u; info[2] = mode == LIT_HUF ? kind : 0u;
    if (mode == LIT_RAW) { const uint32_t h = lit_hdr_plain(o, 0, n); memcpy(o + h, lit, n); return h + n; }
    /* weights, codes: the cells of weight w start behind those of the lower weights, 1 << (w - 1) a symbol, the symbols in order */
    uint32_t cnt[16] = {0}, rstart[16] = {0}, seen[16] = {0};
    for (uint32_t s = 0; s < 256u; s++) cnt[wt[s]]++;
    for (uint32_t w = 2; w <= 12u; w++) rstart[w] = rstart[w - 1] + (cnt[w - 1] << (w - 2u));
    for (uint32_t s = 0; s < 256u; s++) if (wt[s]) code[s] = (rstart[wt[s]] >> (wt[s] - 1u)) + seen[wt[s]]++;
    const uint32_t hl = lit_hdr_huf_len(n), comp = best - hl, fmt = streams == 1u ? 0u : hl == 4u ? 2u : 3u;
    const uint32_t sb = hl == 3u ? 10u : hl == 4u ? 14u : 18u;
    const uint64_t hv = 2u | fmt << 2 | (uint64_t)n << 4 | (uint64_t)comp << (4u + sb);
    for (uint32_t k = 0; k < hl; k++) o[k] = (uint8_t)(hv >> (8u * k));
    uint32_t at = hl;
    if (kind == 2u) { o[at++] = (uint8_t)fse; memcpy(o + at, wout, fse); at += fse; }
    else {
        o[at++] = (uint8_t)(127u + top);
        for (uint32_t s = 0; s < top; s += 2u) o[at++] = (uint8_t)(wt[s] << 4 | (s + 1u < top ? wt[s + 1u] : 0u));
    }
    if (streams == 4u) for (uint32_t q = 0; q < 3u; q++) { o[at++] = (uint8_t)sbytes[q]; o[at++] = (uint8_t)(sbytes[q] >> 8); }
    for (uint32_t q = 0; q < streams; q++) {
        const uint32_t a = streams == 1u ? 0u : q * seg, b = streams == 1u ? n : (q == 3u ? n : a + seg);
        bw_t w = {o + at, 0, 0, 0};
        for (uint32_t i = b; i-- > a;) put(&w, code[lit[i]], lens[lit[i]]);
        close_stream(&w);
        at += (uint32_t)w.pos;
    }
    return at;
}

/* ---- one piece as a Compressed block's content into o (room for 2 n + 1024).  prev: the frame's newest offset, advanced.  Returns the
 * length.  info: 0 literal mode, 1 streams, 2 tree kind, 3 / 4 / 5 LL / OF / ML mode, 6 sequences, 7 literals, 8 bits in the sequence
 * stream's last byte before the final bit */
static uint32_t put_compressed(uint8_t* o, const uint8_t* in, uint32_t n, uint32_t* prev, uint32_t* info) {
    zrec_t* rec = (zrec_t*)malloc(sizeof(zrec_t) * (n / 4u + 2u));
    const uint32_t nr = zse_model_records(in, n, (uint32_t*)rec), nseq = nr - 1u;
    uint8_t* lit = (uint8_t*)malloc(n + 1u);
    uint32_t nlit = 0;
    for (uint32_t r = 0; r < nr; r++) { memcpy(lit + nlit, in + rec[r].lit0, rec[r].lit); nlit += rec[r].lit; }
    uint32_t at = put_literals(o, lit, nlit, info);
    info[3] = info[4] = info[5] = 0; info[6] = nseq; info[7] = nlit; info[8] = 0;
    /* the count: one byte below 128, two below 0x7F00 — a piece of 64 KiB holds at most 16 384 matches of four bytes, so the
     * three-byte form is never needed */
    if (nseq < 128u) o[at++] = (uint8_t)nseq;
    else { o[at++] = (uint8_t)((nseq >> 8) + 0x80u); o[at++] = (uint8_t)nseq; }
    if (nseq != 0u) {
        uint8_t* llc = (uint8_t*)malloc(nseq), *ofc = (uint8_t*)malloc(nseq), *mlc = (uint8_t*)malloc(nseq);
        uint32_t* ofv = (uint32_t*)malloc(4u * nseq);
        uint32_t hl[36] = {0}, ho[32] = {0}, hm[53] = {0};
        for (uint32_t i = 0; i < nseq; i++) {
            ofv[i] = (rec[i].lit > 0u && rec[i].dist == *prev) ? 1u : rec[i].dist + 3u;
            *prev = rec[i].dist;
            llc[i] = (uint8_t)code_of(rec[i].lit, kLLBase, 36); ofc[i] = (uint8_t)hb(ofv[i]); mlc[i] = (uint8_t)code_of(rec[i].mlen, kMLBase, 53);
            hl[llc[i]]++; ho[ofc[i]]++; hm[mlc[i]]++;
        }
        /* each table: RLE when one code is used; else FSE_Compressed when its estimated bits (1 / 256 bit a unit: the description's exact
         * bits and every code's cost from its normalized count) are below the predefined distribution's; else Predefined */
        ctab_t tab[3];
        const uint32_t* hist[3] = {hl, ho, hm};
        const int8_t* def[3] = {kLLNorm, kOFNorm, kMLNorm};
        const uint32_t nsyms[3] = {36, 32, 53}, defsyms[3] = {36, 29, 53}, deflog[3] = {6, 5, 6}, maxlog[3] = {9, 8, 9}, first[3] = {llc[0], ofc[0], mlc[0]};
        uint8_t nc[3][96];
        uint32_t mode[3], ncb[3] = {0, 0, 0};
        for (int t = 0; t < 3; t++) {
            int16_t norm[64];
            uint32_t used = 0, top = 0, pre = 0, fse = 0, log = deflog[t];
            for (uint32_t c = 0; c < nsyms[t]; c++) if (hist[t][c]) { used++; top = c; }
            if (used == 1u) { mode[t] = 1; tab[t].rle = 1; tab[t].log = 0; continue; }
            const uint32_t flog = zsf_pick_log(maxlog[t], used, nseq);
            zsf_normalise(hist[t], top + 1u, nseq, flog, norm);
            ncb[t] = zsf_ncount(norm, top + 1u, flog, nc[t], 96);
            fse = ncb[t] * 8u * 256u;
            for (uint32_t c = 0; c <= top; c++) if (hist[t][c]) {
                fse += hist[t][c] * zsf_cost((uint32_t)norm[c], flog);
                pre += hist[t][c] * zsf_cost((uint32_t)(def[t][c] < 0 ? 1 : def[t][c]), deflog[t]);
            }
            mode[t] = fse < pre ? 2u : 0u;
            if (mode[t] == 0u) { for (uint32_t c = 0; c < defsyms[t]; c++) norm[c] = def[t][c]; top = defsyms[t] - 1u; ncb[t] = 0; } else log = flog;
            fse_ctab(&tab[t], norm, top + 1u, log);
        }
        info[3] = mode[0]; info[4] = mode[1]; info[5] = mode[2];
        o[at++] = (uint8_t)(mode[0] << 6 | mode[1] << 4 | mode[2] << 2);
        for (int t = 0; t < 3; t++) {
            if (mode[t] == 1u) o[at++] = (uint8_t)first[t];
            if (mode[t] == 2u) { memcpy(o + at, nc[t], ncb[t]); at += ncb[t]; }
        }
#define tl tab[0]
#define to tab[1]
#define tm tab[2]
        bw_t w = {o + at, 0, 0, 0};
        cst_t sm, so, sl;
        const uint32_t z = nseq - 1u;
        st_init(&sm, &tm, mlc[z]); st_init(&so, &to, ofc[z]); st_init(&sl, &tl, llc[z]);
        put(&w, rec[z].lit - kLLBase[llc[z]], kLLBits[llc[z]]);
        put(&w, rec[z].mlen - kMLBase[mlc[z]], kMLBits[mlc[z]]);
        put(&w, ofv[z] - (1u << ofc[z]), ofc[z]);
        for (uint32_t i = z; i-- > 0u;) {
            st_put(&w, &so, ofc[i]); st_put(&w, &sm, mlc[i]); st_put(&w, &sl, llc[i]);
            put(&w, rec[i].lit - kLLBase[llc[i]], kLLBits[llc[i]]);
            put(&w, rec[i].mlen - kMLBase[mlc[i]], kMLBits[mlc[i]]);
            put(&w, ofv[i] - (1u << ofc[i]), ofc[i]);
        }
        st_flush(&w, &sm); st_flush(&w, &so); st_flush(&w, &sl);
        info[8] = close_stream(&w);
        at += (uint32_t)w.pos;
#undef tl
#undef to
#undef tm
        free(llc); free(ofc); free(mlc); free(ofv);
    }
    free(rec); free(lit);
    return at;
}

/* ---- XXH64, seed 0 ------------------------------------------------------------------------------------------------------------------- */
#define P1 0x9E3779B185EBCA87ull
#define P2 0xC2B2AE3D27D4EB4Full
#define P3 0x165667B19E3779F9ull
#define P4 0x85EBCA77C2B2AE63ull
#define P5 0x27D4EB2F165667C5ull
static uint64_t rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
static uint64_t xround(uint64_t a, uint64_t v) { return rotl(a + v * P2, 31) * P1; }
static uint64_t ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
uint64_t zse_model_xxh64(const uint8_t* p, uint64_t n) {
    uint64_t h, at = 0;
    if (n >= 32u) {
        uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
        for (; at + 32u <= n; at += 32u) for (int j = 0; j < 4; j++) v[j] = xround(v[j], ld64(p + at + 8 * j));
        h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
        for (int j = 0; j < 4; j++) h = (h ^ xround(0, v[j])) * P1 + P4;
    } else h = P5;
    h += n;
    for (; at + 8u <= n; at += 8u) { h ^= xround(0, ld64(p + at)); h = rotl(h, 27) * P1 + P4; }
    if (at + 4u <= n) { h ^= (uint64_t)ld32(p + at) * P1; h = rotl(h, 23) * P2 + P3; at += 4u; }
    for (; at < n; at++) { h ^= p[at] * P5; h = rotl(h, 11) * P1; }
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

/* ---- the frame ----------------------------------------------------------------------------------------------------------------------- */
static uint32_t head_bytes(uint64_t n) { return n <= 255u ? 6u : n <= 65536u ? 7u : n <= 65791u ? 8u : 10u; }
/* exact worst case: every piece a Raw block.  <= n + 3 (n / 65536 + 1) + 14 */
uint64_t zse_model_bound(uint64_t n, uint32_t flags) {
    if ((flags & ~1u) || n > ZIN_MAX) return 0;
    const uint64_t blocks = n == 0u ? 1u : (n + ZPIECE - 1u) / ZPIECE;
    return head_bytes(n) + 3u * blocks + n + ((flags & 1u) ? 4u : 0u);
}

#define ZINFO 12      /* words of the report per piece: 0 .. 8 put_compressed's, 9 the block type (0 Raw, 1 RLE, 2 Compressed), 10 the depth of the
                       * literals' unlimited Huffman tree, 11 the distinct literal bytes (both of a Huffman-coded section) */

/* The frame of one input.  out must hold zse_model_bound(n, flags) + 8 bytes whatever cap is; the result is the frame's length, or
 * CJ_E_OUT_TOO_SMALL when it is above cap.  report (may be NULL): ZINFO words per piece */
int64_t zse_model_compress(const uint8_t* in, uint64_t n, uint32_t flags, uint8_t* out, uint64_t cap, uint32_t* report) {
    if (n > ZIN_MAX) return ZE_INPUT_TOO_LARGE;
    uint64_t at = 0;
    const uint32_t cks = flags & 1u;
    out[at++] = 0x28; out[at++] = 0xB5; out[at++] = 0x2F; out[at++] = 0xFD;
    if (n <= 255u) { out[at++] = (uint8_t)(0x20u | cks << 2); out[at++] = (uint8_t)n; }
    else if (n <= 65536u) { out[at++] = (uint8_t)(0x60u | cks << 2); out[at++] = (uint8_t)(n - 256u); out[at++] = (uint8_t)((n - 256u) >> 8); }
    else if (n <= 65791u) { out[at++] = (uint8_t)(0x40u | cks << 2); out[at++] = 0x30; out[at++] = (uint8_t)(n - 256u); out[at++] = (uint8_t)((n - 256u) >> 8); }
    else { out[at++] = (uint8_t)(0x80u | cks << 2); out[at++] = 0x30; for (int k = 0; k < 4; k++) out[at++] = (uint8_t)(n >> (8 * k)); }
    const uint64_t np = n == 0u ? 1u : (n + ZPIECE - 1u) / ZPIECE;
    uint8_t* tmp = (uint8_t*)malloc(2u * ZPIECE + 1024u);
    uint32_t prev = 1;
    for (uint64_t p = 0; p < np; p++) {
        const uint8_t* pin = in + p * ZPIECE;
        const uint32_t pn = (uint32_t)(n - p * ZPIECE < ZPIECE ? n - p * ZPIECE : ZPIECE), last = p + 1u == np;
        uint32_t info[ZINFO] = {0}, type = 0, size = pn, same = pn != 0u;
        for (uint32_t i = 1; i < pn; i++) if (pin[i] != pin[0]) { same = 0; break; }
        if (same) type = 1;
        else if (pn != 0u) {
            uint32_t pv = prev;
            const uint32_t c = put_compressed(tmp, pin, pn, &pv, info);
            if (c < pn) { type = 2; size = c; prev = pv; }
            else memset(info, 0, sizeof info);            /* (the report says what was written) */
        }
        const uint32_t h = last | type << 1 | size << 3;
        out[at++] = (uint8_t)h; out[at++] = (uint8_t)(h >> 8); out[at++] = (uint8_t)(h >> 16);
        if (type == 0) { memcpy(out + at, pin, pn); at += pn; }
        else if (type == 1) out[at++] = pin[0];
        else { memcpy(out + at, tmp, size); at += size; }
        info[9] = type;
        if (report) memcpy(report + ZINFO * p, info, sizeof info);
    }
    free(tmp);
    if (cks) { const uint32_t x = (uint32_t)zse_model_xxh64(in, n); for (int k = 0; k < 4; k++) out[at++] = (uint8_t)(x >> (8 * k)); }
    return at <= cap ? (int64_t)at : ZE_OUT_TOO_SMALL;
}
