// blosclz_decode.hip — BloscLZ stream decoder for gfx950, one wavefront per stream (the streams of Blosc chunks whose compressor
// format is 0: blosc_batch.hip with CJ_BLOSC_FLAG_READ_BLOSCLZ).
//
// BloscLZ is a byte-aligned LZ77 of the FastLZ family; accept/reject rules follow c-blosc 1.21's blosclz_decompress:
//   control byte < 32    a literal run of ctrl + 1 bytes; the first control byte of a stream is taken & 31 (a stream opens with literals)
//   control byte >= 32   a match: len = (ctrl >> 5) - 1, extended by bytes while they are 255 when it is 6, + 3; distance =
//                        ((ctrl & 31) << 8) + code + 1, or, when code == 255 and ctrl & 31 == 31, 8191 + a big-endian u16 + 1
//   a match needs two more input bytes behind its control byte (and behind every extension byte, and behind the far form's code);
//   the stream ends when the input is used up behind a literal run or a match, and is good iff it then filled its capacity exactly.
// Unlike LZ4 there is no trailing-literals rule: a stream may end in a match that runs to the last byte of its capacity, and in the
// Blosc scratch the next stream's bytes lie right behind it.  Both copies used here (wave_copy, wave_match_copy) write bytes
// [0, n) of their destination and nothing else, and every length is checked against the capacity before the copy.
//
// Shape: as lz4_wave_decode — the grammar is parsed wave-uniformly out of the 512-byte register window, the lanes only move bytes.
#include "cj_codecs.hpp"
#include "blosclz_wave.hpp"

namespace cj {

// one wavefront per row; a row with out_cap == 0 is not a BloscLZ stream (blosc_batch.hip: a stored stream, copied elsewhere)
__global__ __launch_bounds__(kBlockThreads) void blosclz_decode_kernel(BatchArgs a) {
    const uint32_t row = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (row >= a.n_chunks) return;
    const uint64_t n64 = a.in_len[row], cap64 = a.out_cap[row];
    int64_t r;
    if (cap64 == 0) r = 0;
    else if (n64 > 0x7FFFFFF0ull || cap64 > 0x7FFFFFF0ull) r = CJ_E_CORRUPT;
    else r = blosclz_wave_decode(a.in_base + a.in_off[row], (uint32_t)n64, a.out_base + a.out_off[row], (uint32_t)cap64);
    if (lane_id() == 0) a.result[row] = r;
}

void launch_blosclz_decode(const BatchArgs& a, hipStream_t s) {
    if (a.n_chunks == 0) return;
    hipLaunchKernelGGL(blosclz_decode_kernel, wave_grid(a.n_chunks), dim3(kBlockThreads), 0, s, a);
}

}  // namespace cj
