/* enc2_model.c — scalar CPU statement of the LZ4 and Snappy encoders on the round-based matcher of cramjam_amd/csrc/cj_enc2.hpp (TEST
 * INFRASTRUCTURE).
 *
 * The GPU encoders are specified by this model: the matcher's round and the walk that drives it are enc2_round.h's (the one statement
 * of both, shared with the linked, DEFLATE and Zstandard models); this file puts the walk's matches into the two formats' sequences.
 * tests/test_enc2_gpu.py asserts that the kernels emit exactly these bytes, tests/test_enc2_model.py that the streams decode with the
 * oracle and keep the CPU encoders' ratio — per file of the reference's corpus.
 */
#include "enc2_round.h"

static size_t lz4_put_seq(uint8_t* out, size_t op, const uint8_t* lit_src, uint32_t lit, uint32_t off, uint32_t mlen, int last) {
    const uint32_t mcode = last ? 0u : mlen - 4u;
    out[op++] = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (mcode < 15u ? mcode : 15u));
    if (lit >= 15u) { uint32_t v = lit - 15u; while (v >= 255u) { out[op++] = 255u; v -= 255u; } out[op++] = (uint8_t)v; }
    memcpy(out + op, lit_src, lit); op += lit;
    if (last) return op;
    out[op++] = (uint8_t)off; out[op++] = (uint8_t)(off >> 8);
    if (mcode >= 15u) { uint32_t v = mcode - 15u; while (v >= 255u) { out[op++] = 255u; v -= 255u; } out[op++] = (uint8_t)v; }
    return op;
}

typedef struct { const uint8_t* in; uint8_t* out; size_t op; } put_t;

static void lz4_emit(void* ctx, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen) {
    put_t* w = (put_t*)ctx;
    w->op = lz4_put_seq(w->out, w->op, w->in + lit0, lit, off, mlen, 0);
}

/* LZ4 block (no size prefix); out must hold LZ4_compressBound(n).  R = positions per round (multiple of 256, <= RMAX) */
int64_t enc2_model_lz4(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t R) {
    put_t w = {in, out, 0};
    const uint32_t anchor = n >= 13u ? enc2_walk(in, 0u, n, R, n - 12u, n - 5u, ENC2_NO_MAX_DIST, lz4_emit, &w) : 0u;
    return (int64_t)lz4_put_seq(out, w.op, in + anchor, n - anchor, 0, 0, 1);
}

static size_t sn_put_literal(uint8_t* out, size_t op, const uint8_t* src, uint32_t len) {
    const uint32_t n1 = len - 1u;
    if (n1 < 60u) out[op++] = (uint8_t)(n1 << 2);
    else {
        const uint32_t nb = n1 < 256u ? 1u : n1 < 65536u ? 2u : n1 < 16777216u ? 3u : 4u;
        out[op++] = (uint8_t)((59u + nb) << 2);
        for (uint32_t k = 0; k < nb; k++) out[op++] = (uint8_t)(n1 >> (8u * k));
    }
    memcpy(out + op, src, len);
    return op + len;
}
static size_t sn_put_copy(uint8_t* out, size_t op, uint32_t off, uint32_t len) {
    while (len >= 68u) { out[op++] = (uint8_t)(2u | (63u << 2)); out[op++] = (uint8_t)off; out[op++] = (uint8_t)(off >> 8); len -= 64u; }
    if (len > 64u) { out[op++] = (uint8_t)(2u | (59u << 2)); out[op++] = (uint8_t)off; out[op++] = (uint8_t)(off >> 8); len -= 60u; }
    if (len < 12u && off < 2048u) { out[op++] = (uint8_t)(1u | ((len - 4u) << 2) | ((off >> 8) << 5)); out[op++] = (uint8_t)off; }
    else { out[op++] = (uint8_t)(2u | ((len - 1u) << 2)); out[op++] = (uint8_t)off; out[op++] = (uint8_t)(off >> 8); }
    return op;
}

static void sn_emit(void* ctx, uint32_t lit0, uint32_t lit, uint32_t off, uint32_t mlen) {
    put_t* w = (put_t*)ctx;
    if (lit != 0u) w->op = sn_put_literal(w->out, w->op, w->in + lit0, lit);
    w->op = sn_put_copy(w->out, w->op, off, mlen);
}

/* Snappy raw (with the varint preamble); out must hold 32 + n + n / 6 */
int64_t enc2_model_snappy(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t R) {
    put_t w = {in, out, 0};
    { uint32_t v = n; while (v >= 0x80u) { out[w.op++] = (uint8_t)(v | 0x80u); v >>= 7; } out[w.op++] = (uint8_t)v; }
    const uint32_t anchor = n >= 8u ? enc2_walk(in, 0u, n, R, n - 8u, n, ENC2_NO_MAX_DIST, sn_emit, &w) : 0u;      /* the kernels' position lanes read 8 bytes at a time */
    if (anchor < n) w.op = sn_put_literal(out, w.op, in + anchor, n - anchor);
    return (int64_t)w.op;
}
