/* zstd_fse_enc.h — the serial arithmetic of the Zstandard encoder's FSE stage: the table-log choice, the
 * normaliser, the cost estimate, the NCount writer, the encode-table builder and the FSE-compressed Huffman weights.  Each routine is
 * one lane's work over arrays the caller owns (LDS on the device), in plain C: zstd_enc_wave.hpp and tests/hostsim/zstd_enc_model.c
 * both include this text, so the kernel and the model take the same decisions from the same integers.  What checks it from outside:
 * libzstd and the project's decoder read the frames, tests/zstd_cases.py's read_ncount / fse_cells rebuild the tables.
 * No local array is indexed by a variable (that would be scratch memory on the device).  Not part of the C-ABI. */
#ifndef CJ_ZSTD_FSE_ENC_H
#define CJ_ZSTD_FSE_ENC_H
#include <stdint.h>
#ifndef ZSF_FN
#define ZSF_FN static inline
#endif

ZSF_FN uint32_t zsf_hb(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v | 1u); }

/* the bits of one symbol of normalized count `norm` (1 .. 1 << log) in a table of 1 << log states, in 1 / 256 bit: log - log2(norm)
 * with the logarithm's fraction taken as linear */
ZSF_FN uint32_t zsf_cost(uint32_t norm, uint32_t log) {
    const uint32_t h = zsf_hb(norm);
    return ((log - h) << 8) - (((norm << 8) >> h) - 256u);
}

/* the accuracy log of a table for `total` symbols of which `used` are distinct: two below the total's, at least 5 and what the
 * distinct symbols need, at most maxlog */
ZSF_FN uint32_t zsf_pick_log(uint32_t maxlog, uint32_t used, uint32_t total) {
    const uint32_t need = used > 1u ? zsf_hb(used - 1u) + 1u : 1u, t = zsf_hb(total);
    uint32_t log = t > 2u ? t - 2u : 0u;
    if (log < need) log = need;
    if (log < 5u) log = 5u;
    return log < maxlog ? log : maxlog;
}

/* norm[0, nsym): every used symbol at least 1, the sum exactly 1 << log (used <= 1 << log).  The share rounded down; what is missing
 * goes to the most frequent symbol, what is too much (symbols lifted to 1) comes off the largest count, one at a time */
ZSF_FN void zsf_normalise(const uint32_t* hist, uint32_t nsym, uint32_t total, uint32_t log, int16_t* norm) {
    const uint32_t size = 1u << log;
    uint32_t sum = 0, big = 0, bigc = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const uint32_t c = hist[s];
        uint32_t p = 0;
        if (c != 0u) {
            p = (c << log) / (total ? total : 1u);
            if (p == 0u) p = 1u;
            if (c > bigc) { bigc = c; big = s; }
        }
        norm[s] = (int16_t)p;
        sum += p;
    }
    if (sum <= size) { norm[big] = (int16_t)(norm[big] + (int16_t)(size - sum)); return; }
    for (uint32_t over = sum - size, k = 0; over != 0u && k < 256u; k++, over--) {
        uint32_t m = 0;
        for (uint32_t s = 1; s < nsym; s++) if (norm[s] > norm[m]) m = s;
        if (norm[m] <= 1) return;                                /* (cannot be: used <= size) */
        norm[m] = (int16_t)(norm[m] - 1);
    }
}

/* libzstd's FSE_writeNCount: the description of norm[0, nsym) (nsym = the last used symbol + 1) at accuracy `log` into out[0, cap).
 * Returns its length (what lies beyond cap is counted, not stored) */
ZSF_FN uint32_t zsf_ncount(const int16_t* norm, uint32_t nsym, uint32_t log, uint8_t* out, uint32_t cap) {
    uint64_t acc = 0;
    uint32_t cnt = 0, at = 0, sym = 0, prev0 = 0, nb = log + 1u;
    int32_t remaining = (int32_t)(1u << log) + 1, threshold = (int32_t)(1u << log);
#define ZSF_PUT(v, n) do { acc |= (uint64_t)(v) << cnt; cnt += (n); while (cnt >= 8u) { if (at < cap) out[at] = (uint8_t)acc; at++; acc >>= 8; cnt -= 8u; } } while (0)
    ZSF_PUT(log - 5u, 4u);
    while (sym < nsym && remaining > 1) {
        if (prev0) {
            uint32_t start = sym;
            while (sym < nsym && norm[sym] == 0) sym++;
            if (sym == nsym) break;
            while (sym >= start + 24u) { start += 24u; ZSF_PUT(0xFFFFu, 16u); }
            while (sym >= start + 3u) { start += 3u; ZSF_PUT(3u, 2u); }
            ZSF_PUT(sym - start, 2u);
        }
        int32_t count = norm[sym++];
        const int32_t max = (2 * threshold - 1) - remaining;
        remaining -= count < 0 ? -count : count;
        count++;
        if (count >= threshold) count += max;
        ZSF_PUT((uint32_t)count, nb - (count < max ? 1u : 0u));
        prev0 = count == 1;
        while (remaining < threshold && threshold > 1) { nb--; threshold >>= 1; }
    }
    if (cnt != 0u) { if (at < cap) out[at] = (uint8_t)acc; at++; }
    return at;
}

/* libzstd's FSE_buildCTable: the states of 1 << log cells into st, deltaNbBits / deltaFindState of symbol s at [s & 63].
 * norm[s] = -1: a "less than one" symbol.  cell: 1 << log bytes, cumul: 64 words of the caller's */
ZSF_FN void zsf_table(const int16_t* norm, uint32_t nsym, uint32_t log, uint16_t* st, uint32_t* dnb, int32_t* dfs, uint8_t* cell, uint32_t* cumul) {
    const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    uint32_t high = size - 1u, run = 0, pos = 0, total = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        cumul[s & 63u] = run;
        if (c == -1) { cell[high & 511u] = (uint8_t)s; high--; run += 1u; }
        else run += (uint32_t)c;
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        for (int32_t i = 0; i < c; i++) {
            cell[pos & 511u] = (uint8_t)s;
            pos = (pos + step) & mask;
            for (uint32_t k = 0; k < size && pos > high; k++) pos = (pos + step) & mask;
        }
    }
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t s = cell[u & 511u] & 63u, at = cumul[s];
        cumul[s] = at + 1u;
        st[at & mask] = (uint16_t)(size + u);
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        uint32_t d;
        int32_t f;
        if (c == 0) { d = ((log + 1u) << 16) - size; f = 0; }
        else if (c == -1 || c == 1) { d = (log << 16) - size; f = (int32_t)total - 1; total += 1u; }
        else {
            const uint32_t maxbits = log - zsf_hb((uint32_t)c - 1u);
            d = (maxbits << 16) - ((uint32_t)c << maxbits); f = (int32_t)total - c; total += (uint32_t)c;
        }
        dnb[s & 63u] = d;
        dfs[s & 63u] = f;
    }
}

/* libzstd's HUF_compressWeights: the Huffman weights wt[0, n) (each below 12, n <= 255) as an NCount description at accuracy 5 or 6
 * and one FSE stream of two interleaved states (even places on the first, odd places on the second, the last weight first), into
 * out[0, cap).  Returns the length, or 0 where this form cannot be: fewer than 3 weights, one distinct weight, 128 bytes or more.
 * hist: 16 words, norm: 16, st: 64, dnb / dfs: 64, cell: 64 bytes, cumul: 64 words of the caller's */
ZSF_FN uint32_t zsf_weights(const uint8_t* wt, uint32_t n, uint8_t* out, uint32_t cap, uint32_t* hist, int16_t* norm, uint16_t* st, uint32_t* dnb,
                            int32_t* dfs, uint8_t* cell, uint32_t* cumul) {
    if (n < 3u || n > 255u) return 0u;
    uint32_t used = 0, nsym = 0;
    for (uint32_t s = 0; s < 16u; s++) hist[s] = 0u;
    for (uint32_t i = 0; i < n; i++) hist[wt[i] & 15u] += 1u;
    for (uint32_t s = 0; s < 16u; s++) if (hist[s] != 0u) { used++; nsym = s + 1u; }
    if (used < 2u || nsym > 12u) return 0u;
    const uint32_t log = zsf_pick_log(6u, used, n), mask = (1u << log) - 1u;
    zsf_normalise(hist, nsym, n, log, norm);
    uint32_t at = zsf_ncount(norm, nsym, log, out, cap);
    zsf_table(norm, nsym, log, st, dnb, dfs, cell, cumul);
    uint64_t acc = 0;
    uint32_t cnt = 0, s1 = 0, s2 = 0;
    for (uint32_t i = n; i-- > 0u;) {
        const uint32_t sym = wt[i] & 15u, d = dnb[sym];
        const int32_t f = dfs[sym];
        uint32_t s = (i & 1u) ? s2 : s1;
        if (i + 2u >= n) {                                       /* the last two weights open the two states and leave no bits */
            const uint32_t nb = (d + (1u << 15)) >> 16, v = (nb << 16) - d;
            s = st[(uint32_t)((int32_t)(v >> nb) + f) & mask];
        } else {
            const uint32_t nb = ((s + d) >> 16) & 15u;
            ZSF_PUT(s & ((1u << nb) - 1u), nb);
            s = st[(uint32_t)((int32_t)(s >> nb) + f) & mask];
        }
        if (i & 1u) s2 = s; else s1 = s;
    }
    ZSF_PUT(s2 & mask, log);
    ZSF_PUT(s1 & mask, log);
    ZSF_PUT(1u, 1u);
    if (cnt != 0u) { if (at < cap) out[at] = (uint8_t)acc; at++; }
    return at < 128u && at <= cap ? at : 0u;
}
#undef ZSF_PUT
#endif
