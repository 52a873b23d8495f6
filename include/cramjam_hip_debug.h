/* cramjam_hip_debug.h — test and benchmark utilities that libcramjam_hip.so exports NEXT TO the drop-in ABI of cramjam_hip.h
 * (cramjam_amd/csrc/bench_util.hip and debug counters of the decoders).  A binding of the reference's call sites needs none of them;
 * tests/test_cabi.py pins the two export lists separately. */
#ifndef CRAMJAM_HIP_DEBUG_H
#define CRAMJAM_HIP_DEBUG_H
#include "cramjam_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* n chunks of S bytes at d_out + i*stride = synth-v1(S, first_index + i, seed), generated on the device */
CJ_API int cj_bench_synth_v1(void* d_out, uint64_t stride, uint64_t S, uint64_t first_index, uint64_t n, uint64_t seed, void* stream);
/* *d_mismatches += chunks i in [0, n) with got[got_off[i] .. +S) != want[(i % n_unique)*want_stride .. +S) */
CJ_API int cj_bench_compare(const void* d_got, const uint64_t* d_got_off, const void* d_want, uint64_t want_stride,
                            uint32_t n_unique, uint64_t S, uint32_t n, void* d_mismatches, void* stream);
/* per-phase cycle counters of the workgroup decoder (CJ_FLAG_DEBUG_PROFILE on a device batch): S0, D1, D2, D3, D4, chunks, 6.. sub-phases.
 * out16 must hold SIXTEEN 64-bit slots (128 bytes; it was eight until round 3) */
CJ_API int cj_debug_lds_phase_cycles(unsigned long long* out16, int reset);
/* chunks of the one-kernel decode path (batches with CJ_FLAG_DEBUG_PROFILE) by how their parse finished: from the listed walks, walked P4, walked P3 + P4 (lds_shared.hpp: fused_parse) */
CJ_API int cj_debug_fused_parse_paths(unsigned long long* out3, int reset);
CJ_API long long cj_debug_forwarded_chunks(int reset);            /* chunks / slabs (of calls with CJ_FLAG_DEBUG_PROFILE) that went through the forwarding phase */
CJ_API unsigned long long cj_debug_linked_lds_frames(void);       /* linked-block LZ4 frames decoded by the two-window decoder */
/* large-stream path with its parse stage's absolute sync points handed back (tests compare them with a serial walk) */
CJ_API int64_t cj_debug_big_parse(int codec, uint32_t flags, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                                  uint32_t* sync_pairs, size_t max_pairs, uint64_t* n_seq);

/* bytes of device scratch the engine holds for CJ_FLAG_BIG_CHUNKS batches (list, record areas, summaries, the slab decoder's tables) */
CJ_API uint64_t cj_debug_big_scratch_bytes(cj_engine* e);

/* What the engine's buffers hold between calls (tests/test_scratch_contents_gpu.py).  The list is every DevBuf and
 * PinnedBuf member of cj_engine, by index; e == NULL names the default engine, the one behind the single-buffer and frame calls.
 * _name: the member's name ("d_pmeta"), NULL outside [0, count).  _carries_state: 1 for a buffer that carries state between calls by
 * design ("h_count": the big-chunk counts earlier calls posted) and is therefore never filled, 0 for scratch, -1 outside the list.
 * _fill: every listed buffer that is not a state carrier, over its whole capacity, and the host vector of the batch rows — pattern 0: 0x00
 * bytes, 1: 0xFF bytes, >= 2: a hash of (word index, pattern) in every 32-bit word; it takes the engine's mutexes in their documented order,
 * waits for each scratch's last user, changes no pointer and no capacity, and returns once the bytes are set.  filled[i] (count entries) =
 * the bytes written to buffer i, 0 for one that is not allocated or carries state.  _peek: n bytes of buffer i from offset off, to the host. */
CJ_API int cj_debug_scratch_count(void);
CJ_API const char* cj_debug_scratch_name(int i);
CJ_API int cj_debug_scratch_carries_state(int i);
CJ_API int cj_debug_scratch_fill(cj_engine* e, uint32_t pattern, uint64_t* filled);
CJ_API int cj_debug_scratch_peek(cj_engine* e, int i, uint64_t off, void* out, size_t n);

/* XXH32 (seed 0) of n device streams d_base + d_off[i] .. + d_len[i] into d_out[i] by the frame batches' one-wavefront-per-stream kernel;
 * synchronous (tests hold it to the reference algorithm at every alignment) */
CJ_API int cj_debug_xxh32_device(cj_engine* e, const uint8_t* d_base, const uint64_t* d_off, const uint64_t* d_len, uint32_t* d_out, size_t n);

/* the Blosc filter kernels alone: n_blocks blocks of `bytes` bytes, `stride` apart, from d_src to d_dst (filter: a cj_blosc_filter, applied
 * by a chunk's rules for that block size, or 3: the yardstick, one device-to-device hipMemcpyAsync of the same span; forward = 0: unfilter);
 * synchronous.  ms (may be NULL): the time between two HIP events around the launch alone */
CJ_API int cj_debug_blosc_filter(cj_engine* e, int forward, uint32_t filter, uint32_t typesize, const uint8_t* d_src, uint8_t* d_dst,
                                 uint64_t bytes, uint64_t stride, size_t n_blocks, double* ms);

/* dictionary compress (cj_dict_batch_*): the bytes of staged `dictionary tail | chunk` slots per slice (0 = the default, 1 GiB); returns the
 * previous value.  Tests force more than one slice with it. */
CJ_API uint64_t cj_debug_dict_stage_budget(uint64_t bytes);

/* DEFLATE compress (cj_deflate_compress_batch_*): the bytes of sequence-record slots per slice, one slot of 256.25 KiB per stream in flight
 * (0 = the default, 1280 slots = 320 MiB); returns the previous value.  Tests force more than one slice with it. */
CJ_API uint64_t cj_debug_deflate_slot_budget(uint64_t bytes);
/* BGZF compress (cj_bgzf_batch_* with CJ_OP_COMPRESS): the bytes of bound-sized member slots per turn, one slot of 65 312 bytes per member
 * in flight (0 = the default, 4096 slots); returns the previous value.  Tests force more than one turn with it. */
CJ_API uint64_t cj_debug_bgzf_slot_budget(uint64_t bytes);
/* ORC compress (cj_orc_batch_* with CJ_OP_COMPRESS): the bytes of bound-sized chunk slots per turn, one slot of the codec's bound for
 * block_size bytes per chunk in flight (0 = the default, 256 MiB); returns the previous value.  Tests force more than one turn with it. */
CJ_API uint64_t cj_debug_orc_slot_budget(uint64_t bytes);
/* Parquet compress (cj_parquet_compress_*): the bytes of bound-sized page slots per turn of whole chunks, one 16-byte-rounded slot of
 * the codec's bound per page whose values the codec sees (0 = the default, 256 MiB); a chunk above it takes a turn alone; returns the
 * previous value.  Tests force more than one turn with it. */
CJ_API uint64_t cj_debug_parquet_slot_budget(uint64_t bytes);
/* Zstandard decode (cj_zstd_batch_*): the bytes of literal slots per slice, one slot of 128 KiB + 32 per stream in flight (0 = the
 * default); returns the previous value */
CJ_API uint64_t cj_debug_zstd_slot_budget(uint64_t bytes);
/* Zstandard compress (cj_zstd_compress_batch_*): the bytes of record-and-literal slots per slice, one slot of 320.25 KiB per frame in
 * flight (0 = the default, 1024 slots); returns the previous value.  Tests force more than one slice with it. */
CJ_API uint64_t cj_debug_zstd_enc_slot_budget(uint64_t bytes);
/* The wavefront-per-chunk batches (cj_deflate_batch_*, cj_zstd_batch_*, cj_dict_batch_* and their size queries): the chunks per
 * kernel launch (0 = the default, 2^22: a grid stays below 2^32 threads); returns the previous value.  Tests force more than one
 * launch with it. */
CJ_API uint64_t cj_debug_grid_chunks(uint64_t n);

#ifdef __cplusplus
}
#endif
#endif
