/* enc2_round.h — the one scalar statement of the round-based matcher of cramjam_amd/csrc/cj_enc2.hpp (TEST INFRASTRUCTURE): the round,
 * the walk that drives it, and the walk's output as records.  Static functions only: every model includes this text (enc2_model.c for
 * LZ4 and Snappy, enc2_linked_model.c, deflate_enc_model.c, zstd_enc_model.c), and two of them are linked into one library.
 *
 * A round covers R consecutive positions in BLOCKS of 128 — a block's positions are probed against the hash table and then enter it
 * (all but the followers of a run of equal candidate distances), before the next block is probed (round 6: the table a position sees is
 * at most 128 positions stale; until round 5 a round probed the table as it was when the round began and inserted at its end, only the
 * positions outside the emitted matches — html 4.15 -> 4.48, kppkn.gtb 2.08 -> 2.17, the whole corpus 1.850 -> 1.898 against liblz4's
 * 1.906); only the HEADS of runs of equal candidate distances are verified and become candidates; every head is extended to its true
 * length forwards and backwards; the heads are walked in position order, greedily (the first head whose interval still has four bytes
 * after the previous match ends wins).
 */
#ifndef ENC2_ROUND_H
#define ENC2_ROUND_H
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <stdlib.h>

#define HASH_BITS 13
#define HASH_SIZE (1u << HASH_BITS)
#define RMAX 1024
#define BLOCK 128u
#define ENC2_NO_MAX_DIST 65535u      /* a candidate distance is taken modulo the 64 KiB lap of the 16-bit table: this limit never binds */

static inline uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint32_t hash_slot(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }

typedef struct { uint32_t s, e, off; } sel_t;

/* one round; returns the number of selected matches, updates *cur (end of the last selected match).  max_dist: candidates further
 * back are none (DEFLATE's 32 768), decided where the candidate distance is formed */
static int model_round(const uint8_t* in, uint16_t* tab, uint32_t pos, uint32_t span, uint32_t R, uint32_t last_start, uint32_t limit,
                       uint32_t max_dist, uint32_t* cur_io, sel_t* sel) {
    static uint32_t hs[RMAX], d[RMAX];
    static uint8_t ok[RMAX], valid[RMAX];
    const uint32_t anchor = *cur_io;
    /* block by block: candidates (the slot's position, as a distance modulo the 64 KiB lap of the 16-bit table), then the block's own
     * positions into the table — k-major (lane l owns positions 4 l + k of its group of 256, half a wavefront is a block): the kernel issues
     * one store instruction per (block, k), and within an instruction the highest lane wins a contested slot */
    for (uint32_t b0 = 0; b0 < R; b0 += BLOCK) {
        for (uint32_t i = b0; i < b0 + BLOCK; i++) {
            const uint32_t p = pos + i;
            valid[i] = i < span && p <= last_start;
            ok[i] = 0; d[i] = 0;
            if (!valid[i]) continue;
            hs[i] = hash_slot(ld32(in + p));
            const uint32_t dist = (p - tab[hs[i]]) & 0xffffu;
            if (dist != 0u && dist <= p && dist <= max_dist) d[i] = dist;
        }
        /* ... except the FOLLOWERS: a position whose candidate distance equals its left neighbour's lies inside that neighbour's match if
         * it is one — what the coverage rule of rounds 1-5 kept out of the table, decided here before anything is verified (benchmark
         * data 1.616 -> 1.622, xml 4.31 -> 4.39; the corpus 1.898 -> 1.901) */
        for (uint32_t k = 0; k < 4u; k++)
            for (uint32_t i = b0 + k; i < b0 + BLOCK; i += 4u) {
                if (!valid[i]) continue;
                if (d[i] != 0u && (i & 255u) != 0u && d[i - 1] == d[i]) continue;
                tab[hs[i]] = (uint16_t)(pos + i);
            }
    }
    /* Only the FIRST position of a run of equal distances is verified (its left neighbour IN THE SAME GROUP OF 256 has another distance or
     * no candidate): the positions behind it lie inside its match if it is one, and a candidate dword costs a scattered memory access
     * each — on match-heavy data half of all positions are such followers. */
    for (uint32_t i = 0; i < R; i++) {
        if (d[i] == 0u) continue;
        if ((i & 255u) != 0u && d[i - 1] == d[i]) continue;
        if (ld32(in + pos + i - d[i]) == ld32(in + pos + i)) ok[i] = 1;
    }
    uint32_t cur = anchor;
    int ns = 0;
    for (uint32_t i = 0; i < R; i++) {
        if (!ok[i]) continue;            /* a verified head */
        const uint32_t p = pos + i, c = p - d[i];
        uint32_t e = p + 4u;
        while (e < limit && in[e] == in[e - d[i]]) e++;
        uint32_t s;
        if (p >= cur) {
            uint32_t room = p - cur, bk = 0;
            if (room > c) room = c;
            while (bk < room && in[p - 1u - bk] == in[c - 1u - bk]) bk++;
            s = p - bk;
        } else s = cur;
        if (e < s + 4u || s > last_start) continue;
        sel[ns].s = s; sel[ns].e = e; sel[ns].off = d[i]; ns++;
        cur = e;
    }
    *cur_io = cur;
    return ns;
}

/* The walk: rounds of R positions (a multiple of 256, <= RMAX) from position h to last_start, emit(ctx, lit0, lit, off, mlen) for every
 * selected match in order — literals [lit0, lit0 + lit), then mlen bytes from off back.  Returns the final anchor: what lies behind it
 * is the caller's last literal run.  h is the linked mode's history: positions below h enter the table first, in ascending order (the
 * latest wins a slot), and the walk starts with a full round (the table is indexed already); with none it starts with 64 positions
 * and doubles.  The caller has made sure that last_start and limit do not wrap (n is long enough for one match). */
typedef void (*enc2_emit_fn)(void* ctx, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen);

static uint32_t enc2_walk(const uint8_t* in, uint32_t h, uint32_t n, uint32_t R, uint32_t last_start, uint32_t limit, uint32_t max_dist,
                          enc2_emit_fn emit, void* ctx) {
    uint16_t* tab = (uint16_t*)calloc(HASH_SIZE, 2);
    sel_t* sel = (sel_t*)malloc(sizeof(sel_t) * (RMAX + 2));
    (void)n;
    for (uint32_t q = 0; q < h; q++) tab[hash_slot(ld32(in + q))] = (uint16_t)q;
    uint32_t anchor = h, pos = h, span = h == 0u ? 64u : R;
    while (pos <= last_start) {
        uint32_t cur = anchor;
        const int ns = model_round(in, tab, pos, span, R, last_start, limit, max_dist, &cur, sel);
        uint32_t a = anchor;
        for (int q = 0; q < ns; q++) { emit(ctx, a, sel[q].s - a, sel[q].off, sel[q].e - sel[q].s); a = sel[q].e; }
        anchor = cur;
        const uint32_t round_end = pos + span;
        span = span * 2u < R ? span * 2u : R;
        pos = anchor > round_end ? anchor : round_end;
    }
    free(tab); free(sel);
    return anchor;
}

/* The records of one piece (n <= 65536) as the DEFLATE and Zstandard encoders take them: (literal start, literal count, distance,
 * match length) per match, last_start = n - 8 (the kernels' position lanes read 8 bytes at a time), limit = n; a piece shorter than 8
 * bytes is all literals.  rec must hold n / 4 + 2 records.  Returns their number (the last one carries the final literals and no match) */
typedef struct { uint32_t lit0, lit, dist, mlen; } enc2_rec_t;

static inline void enc2_rec_emit(void* ctx, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen) {
    enc2_rec_t** r = (enc2_rec_t**)ctx;
    *(*r)++ = (enc2_rec_t){lit0, lit, off, mlen};
}
static inline uint32_t enc2_records(const uint8_t* in, uint32_t n, uint32_t max_dist, uint32_t R, uint32_t* rec_out) {
    enc2_rec_t* const rec = (enc2_rec_t*)rec_out;
    enc2_rec_t* r = rec;
    const uint32_t anchor = n >= 8u ? enc2_walk(in, 0u, n, R, n - 8u, n, max_dist, enc2_rec_emit, &r) : 0u;
    *r++ = (enc2_rec_t){anchor, n - anchor, 0u, 0u};
    return (uint32_t)(r - rec);
}

#endif
