/* deflate_enc_model.c — scalar CPU statement of the DEFLATE encoder of cramjam_amd/csrc/deflate_encode.hip (TEST INFRASTRUCTURE;
 * DESIGN.md 5.13).  The kernel and the host build of its entropy stage (sim_deflate_encode.cpp) emit exactly these bytes.
 *
 *   pieces    the input is cut into independent pieces of at most 65 536 bytes; no match crosses a piece
 *   matching  enc2_round.h's round (R = 512) with candidates limited to a distance of 32 768; last_start = n - 8,
 *             limit = n; a piece shorter than 8 bytes is all literals.  A piece becomes records (literal start, literal count,
 *             distance, match length); the last record carries the final literals and no match
 *   symbols   literals, length / distance pairs (a match above 258 is split into pieces of at most 258, none below 3), end of block
 *   codes     Huffman over the used symbols in (count, symbol) order by the two-queue construction (a leaf wins a tie), depths
 *             above the limit folded into it and the Kraft sum repaired one unit at a time (the deepest shorter code gives way);
 *             the lengths go to the symbols in (count, symbol) order, longest first; canonical codes as RFC 1951 3.2.2
 *   header    HLIT / HDIST / HCLEN trimmed; the lengths of both alphabets as one sequence, run-length coded greedily
 *   choice    stored, fixed or dynamic by their exact bit costs at the block's bit position; a tie goes to the simpler block
 *   wrappers  none / zlib (78 01 .. Adler-32) / gzip (fixed 10-byte header .. CRC-32, ISIZE)
 */
#include "enc2_round.h"

#define MAX_DIST 32768u
#define PIECE 65536u
#define E_OUT_TOO_SMALL (-6)

typedef enc2_rec_t rec_t;

/* the records of one piece (n <= 65536); rec must hold n / 4 + 2 records.  Returns their number (the last one has no match) */
uint32_t dfe_model_records(const uint8_t* in, uint32_t n, uint32_t* rec_out) { return enc2_records(in, n, MAX_DIST, 512u, rec_out); }

/* ---- symbols ------------------------------------------------------------------------------------------------------------------- */
static uint32_t n_split(uint32_t m) { return m ? (m + 257u) / 258u : 0u; }
static uint32_t split_len(uint32_t m, uint32_t k, uint32_t j) {
    const uint32_t rem = m - 258u * (k - 1u);
    if (j + 1u == k) return rem < 3u ? 3u : rem;
    if (j + 2u == k && rem < 3u) return 258u - (3u - rem);
    return 258u;
}
static uint32_t ilog2(uint32_t v) { uint32_t r = 0; while (v >>= 1) r++; return r; }
static void len_sym(uint32_t L, uint32_t* sym, uint32_t* xb, uint32_t* xv) {
    const uint32_t l = L - 3u;
    if (L == 258u) { *sym = 285u; *xb = 0; *xv = 0; return; }
    if (l < 8u) { *sym = 257u + l; *xb = 0; *xv = 0; return; }
    const uint32_t e = ilog2(l) - 2u;
    *sym = 257u + 4u * e + 4u + ((l >> e) & 3u); *xb = e; *xv = l & ((1u << e) - 1u);
}
static void dist_sym(uint32_t D, uint32_t* sym, uint32_t* xb, uint32_t* xv) {
    const uint32_t dd = D - 1u;
    if (dd < 4u) { *sym = dd; *xb = 0; *xv = 0; return; }
    const uint32_t hb = ilog2(dd), e = hb - 1u;
    *sym = 2u * hb + ((dd >> e) & 1u); *xb = e; *xv = dd & ((1u << e) - 1u);
}
static uint32_t len_xb(uint32_t s) { return s < 265u || s >= 285u ? 0u : (s - 261u) / 4u; }
static uint32_t dist_xb(uint32_t s) { return s < 4u ? 0u : (s >> 1) - 1u; }
static uint32_t fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

/* ---- length-limited code lengths.  Returns the depth of the unlimited Huffman tree (what the limit had to cut) ------------------------ */
uint32_t dfe_model_build_lens(const uint32_t* hist, uint32_t nsym, uint32_t maxbits, int pad_single, uint8_t* lens) {
    uint32_t order[288], sw[288], iw[288], par[576], idep[288], blc[64];
    uint32_t n = 0;
    memset(lens, 0, nsym);
    for (uint32_t s = 0; s < nsym; s++) if (hist[s]) order[n++] = s;
    for (uint32_t i = 1; i < n; i++) {                   /* ascending (count, symbol) */
        const uint32_t s = order[i];
        uint32_t j = i;
        while (j > 0 && hist[order[j - 1]] > hist[s]) { order[j] = order[j - 1]; j--; }
        order[j] = s;
    }
    if (n == 0) return 0;
    if (n == 1) {                                        /* one code of length 1 (the code-length alphabet: a second one beside it) */
        lens[order[0]] = 1;
        if (pad_single) lens[order[0] == 0u ? 1 : 0] = 1;
        return 1;
    }
    for (uint32_t i = 0; i < n; i++) sw[i] = hist[order[i]];
    uint32_t li = 0, ii = 0;
    for (uint32_t ni = 0; ni + 1u < n; ni++) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; pick++) {
            if (li < n && (ii >= ni || sw[li] <= iw[ii])) { w += sw[li]; par[li] = ni; li++; }
            else { w += iw[ii]; par[288 + ii] = ni; ii++; }
        }
        iw[ni] = w;
    }
    idep[n - 2] = 0;
    for (uint32_t k = n - 2; k-- > 0;) idep[k] = idep[par[288 + k]] + 1u;
    memset(blc, 0, sizeof blc);
    uint32_t deepest = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t d = idep[par[i]] + 1u;
        if (d > deepest) deepest = d;
        if (d > maxbits) d = maxbits;
        blc[d]++;
    }
    uint32_t total = 0;
    for (uint32_t l = 1; l <= maxbits; l++) total += blc[l] << (maxbits - l);
    while (total > (1u << maxbits)) {
        blc[maxbits]--;
        for (uint32_t l = maxbits - 1u; l > 0; l--)
            if (blc[l]) { blc[l]--; blc[l + 1] += 2; break; }
        total--;
    }
    for (uint32_t r = 0; r < n; r++) {                   /* the rarest symbols get the longest codes */
        uint32_t c = 0, len = 1;
        for (uint32_t l = maxbits; l >= 1u; l--) { c += blc[l]; if (r < c) { len = l; break; } }
        lens[order[r]] = (uint8_t)len;
    }
    return deepest;
}

static uint32_t bitrev(uint32_t v, uint32_t n) { uint32_t r = 0; for (uint32_t k = 0; k < n; k++) r |= ((v >> k) & 1u) << (n - 1u - k); return r; }
/* canonical codes, bit-reversed (the stream takes a code from its most significant bit) */
static void canon(const uint8_t* lens, uint32_t nsym, uint32_t maxbits, uint32_t* code) {
    uint32_t cnt[17] = {0}, next[17] = {0};
    for (uint32_t s = 0; s < nsym; s++) cnt[lens[s]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (uint32_t l = 1; l <= maxbits; l++) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (uint32_t s = 0; s < nsym; s++) code[s] = lens[s] ? bitrev(next[lens[s]]++, lens[s]) : 0u;
}

/* ---- the bit writer ---------------------------------------------------------------------------------------------------------------- */
typedef struct { uint8_t* out; uint64_t pos; uint64_t acc; uint32_t cnt; } bw_t;
static void put(bw_t* w, uint32_t v, uint32_t n) {
    w->acc |= (uint64_t)v << w->cnt;
    w->cnt += n;
    while (w->cnt >= 8u) { w->out[w->pos++] = (uint8_t)w->acc; w->acc >>= 8; w->cnt -= 8u; }
}
static void align(bw_t* w) { if (w->cnt) { w->out[w->pos++] = (uint8_t)w->acc; w->acc = 0; w->cnt = 0; } }
static uint64_t bitpos(const bw_t* w) { return 8u * w->pos + w->cnt; }

static const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

/* the run-length coding of a sequence of code lengths: tok[i] = symbol | extra value << 8 */
static uint32_t rle(const uint8_t* seq, uint32_t m, uint16_t* tok) {
    uint32_t nt = 0, i = 0;
    while (i < m) {
        const uint32_t v = seq[i];
        uint32_t run = 1;
        while (i + run < m && seq[i + run] == v) run++;
        i += run;
        if (v == 0u) {
            while (run >= 11u) { const uint32_t r = run < 138u ? run : 138u; tok[nt++] = (uint16_t)(18u | (r - 11u) << 8); run -= r; }
            if (run >= 3u) { tok[nt++] = (uint16_t)(17u | (run - 3u) << 8); run = 0; }
            while (run) { tok[nt++] = 0; run--; }
        } else {
            tok[nt++] = (uint16_t)v; run--;
            while (run >= 3u) { const uint32_t r = run < 6u ? run : 6u; tok[nt++] = (uint16_t)(16u | (r - 3u) << 8); run -= r; }
            while (run) { tok[nt++] = (uint16_t)v; run--; }
        }
    }
    return nt;
}
static uint32_t tok_xb(uint32_t s) { return s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u; }

static void put_stored(bw_t* w, const uint8_t* p, uint32_t len, int final) {
    put(w, final ? 1u : 0u, 3);
    align(w);
    put(w, len, 16); put(w, len ^ 0xffffu, 16);
    memcpy(w->out + w->pos, p, len);
    w->pos += len;
}

/* one piece as one block (two stored ones at 65 536 bytes); returns the block type: 0 stored, 1 fixed, 2 dynamic */
static int put_piece(bw_t* w, const uint8_t* in, uint32_t n, int final, uint32_t* depth) {
    rec_t* rec = (rec_t*)malloc(sizeof(rec_t) * (n / 4u + 2u));
    const uint32_t nr = dfe_model_records(in, n, (uint32_t*)rec);
    uint32_t hl[288] = {0}, hd[32] = {0};
    for (uint32_t r = 0; r < nr; r++) {
        for (uint32_t j = 0; j < rec[r].lit; j++) hl[in[rec[r].lit0 + j]]++;
        const uint32_t k = n_split(rec[r].mlen);
        for (uint32_t j = 0; j < k; j++) {
            uint32_t s, xb, xv;
            len_sym(split_len(rec[r].mlen, k, j), &s, &xb, &xv); hl[s]++;
            dist_sym(rec[r].dist, &s, &xb, &xv); hd[s]++;
        }
    }
    hl[256]++;
    uint8_t ll[288] = {0}, dl[32] = {0}, seq[320], cl[19];
    const uint32_t d0 = dfe_model_build_lens(hl, 286, 15, 0, ll), d1 = dfe_model_build_lens(hd, 30, 15, 0, dl);
    if (depth) { if (d0 > depth[0]) depth[0] = d0; if (d1 > depth[1]) depth[1] = d1; }
    uint32_t hlit = 286, hdist = 30, hclen = 19;
    while (hlit > 257u && ll[hlit - 1] == 0) hlit--;
    while (hdist > 1u && dl[hdist - 1] == 0) hdist--;
    memcpy(seq, ll, hlit); memcpy(seq + hlit, dl, hdist);
    uint16_t tok[320];
    const uint32_t nt = rle(seq, hlit + hdist, tok);
    uint32_t hc[19] = {0};
    for (uint32_t i = 0; i < nt; i++) hc[tok[i] & 0xffu]++;
    dfe_model_build_lens(hc, 19, 7, 1, cl);
    while (hclen > 4u && cl[kClOrder[hclen - 1]] == 0) hclen--;
    uint64_t dyn = 3u + 14u + 3u * hclen, fix = 3u;
    for (uint32_t i = 0; i < nt; i++) dyn += cl[tok[i] & 0xffu] + tok_xb(tok[i] & 0xffu);
    for (uint32_t s = 0; s < 286u; s++) { dyn += (uint64_t)hl[s] * (ll[s] + len_xb(s)); fix += (uint64_t)hl[s] * (fixed_len(s) + len_xb(s)); }
    for (uint32_t s = 0; s < 30u; s++) { dyn += (uint64_t)hd[s] * (dl[s] + dist_xb(s)); fix += (uint64_t)hd[s] * (5u + dist_xb(s)); }
    const uint32_t pad = (uint32_t)((8u - (bitpos(w) + 3u) % 8u) % 8u);
    uint64_t sto = 3u + pad + 32u + 8u * (uint64_t)n;
    if (n == PIECE) sto += 3u + 5u + 32u;
    int type;
    if (sto <= fix && sto <= dyn) {
        type = 0;
        if (n == PIECE) { put_stored(w, in, 65535u, 0); put_stored(w, in + 65535u, 1u, final); }
        else put_stored(w, in, n, final);
    } else {
        uint32_t lc[288], dc[32], cc[19];
        type = fix <= dyn ? 1 : 2;
        if (type == 1) {
            for (uint32_t s = 0; s < 288u; s++) ll[s] = (uint8_t)fixed_len(s);
            for (uint32_t s = 0; s < 32u; s++) dl[s] = 5;
        }
        canon(ll, 288, 15, lc); canon(dl, 32, 15, dc);
        put(w, (final ? 1u : 0u) | (uint32_t)type << 1, 3);
        if (type == 2) {
            canon(cl, 19, 7, cc);
            put(w, hlit - 257u, 5); put(w, hdist - 1u, 5); put(w, hclen - 4u, 4);
            for (uint32_t k = 0; k < hclen; k++) put(w, cl[kClOrder[k]], 3);
            for (uint32_t i = 0; i < nt; i++) {
                const uint32_t s = tok[i] & 0xffu;
                put(w, cc[s], cl[s]);
                put(w, tok[i] >> 8, tok_xb(s));
            }
        }
        for (uint32_t r = 0; r < nr; r++) {
            for (uint32_t j = 0; j < rec[r].lit; j++) { const uint32_t b = in[rec[r].lit0 + j]; put(w, lc[b], ll[b]); }
            const uint32_t k = n_split(rec[r].mlen);
            for (uint32_t j = 0; j < k; j++) {
                uint32_t s, xb, xv;
                len_sym(split_len(rec[r].mlen, k, j), &s, &xb, &xv);
                put(w, lc[s], ll[s]); put(w, xv, xb);
                dist_sym(rec[r].dist, &s, &xb, &xv);
                put(w, dc[s], dl[s]); put(w, xv, xb);
            }
        }
        put(w, lc[256], ll[256]);
    }
    free(rec);
    return type;
}

uint64_t dfe_model_bound(uint64_t n, int wrap) {
    const uint64_t full = n / PIECE, rest = (n % PIECE != 0u || n == 0u) ? 1u : 0u;
    return n + 10u * full + 5u * rest + (wrap == 1 ? 6u : wrap == 2 ? 18u : 0u);
}

static uint32_t crc32_bytes(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u); }
    return ~c;
}
static uint32_t adler32_bytes(const uint8_t* p, uint64_t n) {
    uint32_t a = 1, b = 0;
    for (uint64_t i = 0; i < n; i++) { a = (a + p[i]) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}

/* The stream of one input.  out must hold dfe_model_bound(n, wrap) + 8 bytes whatever cap is; the result is the stream's length, or
 * CJ_E_OUT_TOO_SMALL when it is above cap.  types (may be NULL): the block type of every piece; depth (may be NULL, three words):
 * depth[0] / [1] = the deepest unlimited Huffman tree of a literal/length / distance alphabet of the pieces, depth[2] = the bits of
 * the last block in the stream's last byte before the trailer (0: it ends on a byte boundary) */
int64_t dfe_model_compress(const uint8_t* in, uint64_t n, int wrap, uint8_t* out, uint64_t cap, uint8_t* types, uint32_t* depth) {
    bw_t w = {out, 0, 0, 0};
    if (depth) depth[0] = depth[1] = 0;
    if (wrap == 1) { put(&w, 0x78, 8); put(&w, 0x01, 8); }
    if (wrap == 2) { const uint8_t h[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff}; for (int i = 0; i < 10; i++) put(&w, h[i], 8); }
    const uint64_t np = n == 0u ? 1u : (n + PIECE - 1u) / PIECE;
    for (uint64_t p = 0; p < np; p++) {
        const uint64_t at = p * PIECE;
        const uint32_t pn = (uint32_t)(n - at < PIECE ? n - at : PIECE);
        const int t = put_piece(&w, in + at, pn, p + 1u == np, depth);
        if (types) types[p] = (uint8_t)t;
    }
    if (depth) depth[2] = w.cnt;
    align(&w);
    if (wrap == 1) { const uint32_t a = adler32_bytes(in, n); for (int k = 3; k >= 0; k--) put(&w, (a >> (8 * k)) & 0xffu, 8); }
    if (wrap == 2) { put(&w, crc32_bytes(in, n), 32); put(&w, (uint32_t)n, 32); }
    return w.pos <= cap ? (int64_t)w.pos : E_OUT_TOO_SMALL;
}
