/* enc2_linked_model.c — the scalar model of the LINKED-block mode of the LZ4 encoder (TEST INFRASTRUCTURE; cramjam_amd/csrc/lz4_encode.hip
 * with kFlagLinkedEnc, what cj_lz4_frame_compress_linked writes per 64 KiB block).
 *
 * A linked block may refer to the 64 KiB of input before it.  `in` points h <= 65536 bytes before the block, n counts history plus block:
 *   - every history position q < h enters the table first, in ascending order (the latest position wins a slot); hash(ld32(in + q)) may
 *     read up to 3 bytes into the block;
 *   - then the rounds of enc2_model_lz4 run from pos = anchor = h — a full round at once when there is history (the table is indexed
 *     already, as for the split pieces of large.hip), 64 positions first when there is none; candidates may lie in the history (dist <= p),
 *     backward extension never passes the anchor, last_start and limit are measured from the end of the block;
 *   - a block shorter than 13 bytes is one literal run.
 * With h = 0 the output is enc2_model_lz4's.  tests/test_linked_frames_gpu.py holds the kernel to these bytes. */
#include "enc2_model.c"

int64_t enc2_model_lz4_linked(const uint8_t* in, uint32_t h, uint32_t n, uint8_t* out, uint32_t R) {
    size_t op = 0;
    uint32_t anchor = h;
    if (h > 65536u || h > n) return -1;
    if (n - h >= 13u) {
        uint16_t* tab = (uint16_t*)calloc(HASH_SIZE, 2);
        sel_t* sel = (sel_t*)malloc(sizeof(sel_t) * (RMAX + 2));
        for (uint32_t q = 0; q < h; q++) tab[hash_slot(ld32(in + q))] = (uint16_t)q;
        const uint32_t last_start = n - 12u, limit = n - 5u;
        uint32_t pos = h, span = h == 0u ? 64u : R;
        while (pos <= last_start) {
            uint32_t cur = anchor;
            const int ns = model_round(in, n, tab, pos, span, R, last_start, limit, &cur, sel);
            uint32_t a = anchor;
            for (int q = 0; q < ns; q++) { op = lz4_put_seq(out, op, in + a, sel[q].s - a, sel[q].off, sel[q].e - sel[q].s, 0); a = sel[q].e; }
            anchor = cur;
            const uint32_t round_end = pos + span;
            span = span * 2u < R ? span * 2u : R;
            pos = anchor > round_end ? anchor : round_end;
        }
        free(tab); free(sel);
    }
    op = lz4_put_seq(out, op, in + anchor, n - anchor, 0, 0, 1);
    return (int64_t)op;
}
