/* enc2_linked_model.c — the scalar model of the LINKED-block mode of the LZ4 encoder (TEST INFRASTRUCTURE; cramjam_amd/csrc/lz4_encode.hip
 * with kFlagLinkedEnc, what cj_lz4_frame_compress_linked writes per 64 KiB block).
 *
 * A linked block may refer to the 64 KiB of input before it.  `in` points h <= 65536 bytes before the block, n counts history plus block:
 *   - every history position q < h enters the table first, in ascending order (the latest position wins a slot); hash(ld32(in + q)) may
 *     read up to 3 bytes into the block;
 *   - then the rounds of enc2_model_lz4 run from pos = anchor = h — a full round at once when there is history (the table is indexed
 *     already, as for the split pieces of large.hip), 64 positions first when there is none; candidates may lie in the history (dist <= p),
 *     backward extension never passes the anchor, last_start and limit are measured from the end of the block (enc2_round.h's walk with
 *     its history argument);
 *   - a block shorter than 13 bytes is one literal run.
 * With h = 0 the output is enc2_model_lz4's.  tests/test_linked_frames_gpu.py holds the kernel to these bytes. */
#include "enc2_model.c"

int64_t enc2_model_lz4_linked(const uint8_t* in, uint32_t h, uint32_t n, uint8_t* out, uint32_t R) {
    if (h > 65536u || h > n) return -1;
    put_t w = {in, out, 0};
    const uint32_t anchor = n - h >= 13u ? enc2_walk(in, h, n, R, n - 12u, n - 5u, ENC2_NO_MAX_DIST, lz4_emit, &w) : h;
    return (int64_t)lz4_put_seq(out, w.op, in + anchor, n - anchor, 0, 0, 1);
}
