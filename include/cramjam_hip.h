/*
 * cramjam_hip.h — the C-ABI of libcramjam_hip.so: an MI355X (gfx950) batched block-codec engine for
 * cramjam's LZ4-block and Snappy-raw hot path.
 *
 * This is the drop-in boundary.  The reference (milesgranger/cramjam) has no plugin registry; its
 * hot path sits behind the crate-call boundary between src/{lz4,snappy}.rs and libcramjam, i.e.
 * plain functions over borrowed byte slices.  Each export below names the reference call site it
 * replaces (paths relative to the reference repository).  A Rust/pyo3 host binds them with
 * `extern "C"` exactly as INTEGRATION.md shows; the Python host in cramjam_amd/ binds the same
 * symbols.  No torch / HIP types appear in any signature: pointers, sizes and ints only.
 *
 * Conventions
 *   - return int64_t >= 0: bytes written / decoded;  < 0: one of CJ_E_* (cj_strerror gives the
 *     message the reference's Rust error would have carried).
 *   - inputs are borrowed for the duration of the call, never retained or freed; outputs are
 *     written into caller memory (the host layer allocates with the bound/len helpers and truncates).
 *   - every export is thread-safe and re-entrant (the reference calls with the GIL released,
 *     src/lz4.rs:84,126,163,205; src/snappy.rs:57,75,97,106).
 *   - all codec arithmetic (and the Snappy framing CRC-32C) runs in HIP kernels on the GPU.  There is NO CPU
 *     fallback: without a usable HIP device every compute entry point returns CJ_E_NO_DEVICE.  The one
 *     piece of checksum arithmetic on the host is the single-frame LZ4 exports' XXH32 (a serial recurrence per
 *     frame; it runs on a thread concurrently with the device batch — see DESIGN.md §5.5).  The frame batches
 *     (cj_frame_batch_*) compute XXH32 on the device: their streams may have no host copy.
 */
#ifndef CRAMJAM_HIP_H
#define CRAMJAM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: exactly the functions declared here are exported */
#define CJ_API __attribute__((visibility("default")))

#define CJ_ABI_VERSION 1

/* ---- error codes ---- */
#define CJ_E_INPUT_TOO_LARGE   (-1)  /* lz4 crate: "Compression input too long." */
#define CJ_E_COMPRESS_FAILED   (-2)  /* lz4 crate: "Compression failed" (output buffer too small) */
#define CJ_E_NO_PREFIX         (-3)  /* lz4 crate: "Source buffer must at least contain size prefix." */
#define CJ_E_NEG_PREFIX        (-4)  /* lz4 crate: "Parsed size prefix in buffer must not be negative." */
#define CJ_E_PREFIX_TOO_BIG    (-5)  /* lz4 crate: "Given size parameter is too big" */
#define CJ_E_OUT_TOO_SMALL     (-6)  /* lz4 crate: "buffer isn't large enough to hold decompressed data" */
#define CJ_E_CORRUPT           (-7)  /* lz4 crate: "Decompression failed. Input invalid or too long?" */
#define CJ_E_SNAPPY_EMPTY      (-8)  /* snap::Error::Empty */
#define CJ_E_SNAPPY_HEADER     (-9)  /* snap::Error::Header */
#define CJ_E_SNAPPY_TOO_BIG    (-10) /* snap::Error::TooBig */
#define CJ_E_SNAPPY_BUF_SMALL  (-11) /* snap::Error::BufferTooSmall */
#define CJ_E_SNAPPY_CORRUPT    (-12) /* snap::Error::{Literal,CopyRead,CopyWrite,Offset,HeaderMismatch} */
#define CJ_E_FRAME_EOF         (-13) /* io::ErrorKind::UnexpectedEof "failed to fill whole buffer" (truncated framed stream) */
#define CJ_E_FRAME_WRITE       (-14) /* io::ErrorKind::WriteZero "failed to write whole buffer" (framed output does not fit) */
#define CJ_E_SNAPPY_STREAM_HEADER (-15) /* snap::Error::{StreamHeader,StreamHeaderMismatch} */
#define CJ_E_SNAPPY_CHUNK_TYPE (-16) /* snap::Error::UnsupportedChunkType */
#define CJ_E_SNAPPY_CHUNK_LEN  (-17) /* snap::Error::UnsupportedChunkLength */
#define CJ_E_SNAPPY_CHECKSUM   (-18) /* snap::Error::Checksum */
#define CJ_E_LZ4F_FRAME_TYPE    (-20) /* LZ4F ERROR_frameType_unknown (bad magic number) */
#define CJ_E_LZ4F_HEADER        (-21) /* LZ4F ERROR_headerVersion_wrong / reservedFlag_set / headerChecksum_invalid */
#define CJ_E_LZ4F_BLOCK_SIZE    (-22) /* LZ4F ERROR_maxBlockSize_invalid */
#define CJ_E_LZ4F_BLOCK_CHECKSUM (-23) /* LZ4F ERROR_blockChecksum_invalid */
#define CJ_E_LZ4F_CONTENT_CHECKSUM (-24) /* LZ4F ERROR_contentChecksum_invalid */
#define CJ_E_LZ4F_CONTENT_SIZE  (-25) /* LZ4F ERROR_frameSize_wrong */
#define CJ_E_LZ4F_INCOMPLETE    (-26) /* lz4 crate Decoder::finish: "Finish runned before read end of compressed stream" */
#define CJ_E_LZ4F_DECOMPRESS    (-27) /* LZ4F ERROR_decompressionFailed (malformed block) */
#define CJ_E_BLOSC_HEADER       (-30) /* Blosc chunk: malformed header, block table or stream word (c-blosc returns -1) */
#define CJ_E_BLOSC_UNSUPPORTED  (-31) /* Blosc chunk this library does not read or write: see "Blosc chunks" below */
#define CJ_E_DEFLATE_CORRUPT    (-40) /* zlib: "invalid block type" / "invalid stored block lengths" / "too many length or distance symbols" /
                                         "invalid code lengths set" / "invalid bit length repeat" / "invalid code -- missing end-of-block" /
                                         "invalid literal/lengths set" / "invalid distances set" / "invalid literal/length code" /
                                         "invalid distance code" / "invalid distance too far back" */
#define CJ_E_DEFLATE_HEADER     (-41) /* zlib: "incorrect header check" / "unknown compression method" / "invalid window size" /
                                         "unknown header flags set" / "header crc mismatch"; a zlib stream that asks for a preset dictionary */
#define CJ_E_DEFLATE_CHECKSUM   (-42) /* zlib: "incorrect data check" (Adler-32, CRC-32) / "incorrect length check" (gzip ISIZE) */
#define CJ_E_DEFLATE_EOF        (-43) /* zlib: "incomplete or truncated stream" (Z_BUF_ERROR): the input ends inside the stream or its trailer */
#define CJ_E_DEFLATE_TRAILING   (-44) /* bytes behind the stream (zlib leaves them as unused data; one chunk is exactly one stream here) */
#define CJ_E_ZSTD_HEADER        (-50) /* libzstd: prefix_unknown (bad magic, legacy frames included) / frameParameter_unsupported (reserved bit) /
                                         frameParameter_windowTooLarge */
#define CJ_E_ZSTD_CORRUPT       (-51) /* libzstd: corruption_detected (and dictionary_corrupted: Treeless literals before any Huffman table) */
#define CJ_E_ZSTD_CHECKSUM      (-52) /* libzstd: checksum_wrong (the content checksum differs or is cut off) */
#define CJ_E_ZSTD_SRC_SIZE      (-53) /* libzstd: srcSize_wrong (a truncated input, or bytes behind the last frame) */
#define CJ_E_ZSTD_DICT          (-54) /* libzstd: dictionary_wrong (the frame names a dictionary; none is supported) */
#define CJ_E_ORC_HEADER         (-60) /* ORC compression stream: fewer than 3 bytes are left where a chunk header must stand, or a chunk's
                                         length runs past the stream's end */
#define CJ_E_ORC_BLOCK          (-61) /* ORC compression stream: a chunk, original or compressed, holds more than block_size decoded bytes */
#define CJ_E_PARQUET_HEADER     (-70) /* Parquet column chunk: the bytes end inside a page header, a varint is longer than 10 bytes, a wire type is
                                      * unknown or a known field has the wrong one, the nesting of a skipped field is too deep, a required field is
                                      * missing, a size is negative, a V2 page's level lengths exceed either stated size, or a payload runs past the
                                      * chunk's end */
#define CJ_E_PARQUET_SIZE       (-71) /* Parquet column chunk: a page's codec stream decodes cleanly to fewer bytes than its header states */
#define CJ_E_PARQUET_CRC        (-72) /* Parquet column chunk: a page's CRC-32 (verified on request) does not match its header's */
#define CJ_E_PARQUET_TABLE      (-73) /* Parquet writer: the page table is inconsistent — a page type outside {0, 2, 3}, a negative size, level
                                      * lengths on a page that is not V2 or above the page's size, sizes whose sum is not the chunk's length,
                                      * or more rows than 0xFFFFFFF0 */
#define CJ_E_NO_DEVICE         (-100) /* no HIP device / HIP runtime failure (see cj_last_hip_error) */
#define CJ_E_BAD_ARG           (-101)
#define CJ_E_OOM               (-102) /* device or pinned-host allocation failed */

CJ_API const char* cj_strerror(int64_t code);
/* text of the last HIP runtime error seen by the calling thread ("" if none) */
CJ_API const char* cj_last_hip_error(void);
CJ_API int cj_abi_version(void);
/* number of visible HIP devices (0 if none / runtime unusable) */
CJ_API int cj_device_count(void);

/* =====================================================================================
 * Single-buffer entry points — exactly what a pyo3/Rust host would bind in place of the
 * libcramjam calls.  Host pointers.  Run on the default engine of device 0 (of
 * the devices HIP_VISIBLE_DEVICES shows), created lazily.
 * ===================================================================================== */

/* Single-buffer entry points.  A buffer above 64 KiB (input, or announced output) is not run as one serial stream on one
 * wavefront: compress cuts it into 64 KiB pieces, compresses them as a batch and joins them into ONE valid block / raw
 * stream; decompress parses the stream in parallel and decodes it in 64 KiB slabs of output.  Same
 * arguments, results and error codes either way. */

/* src/lz4.rs:228  libcramjam::lz4::block::compress_bound(len, Some(prepend))
 * = LZ4_compressBound(len) (+4 when prepend); 0 when len > 0x7E000000. Pure arithmetic, no device. */
CJ_API size_t cj_lz4_block_compress_bound(size_t len, int prepend);

/* src/lz4.rs:127,206  libcramjam::lz4::block::compress_into(in, out, level, accel, prepend)
 * level/accel: -1 = None.  The reference forwards them but libcramjam always runs the DEFAULT
 * mode, so they do not change the output; accepted and ignored here too.  prepend: -1 = None -> 1. */
CJ_API int64_t cj_lz4_block_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                              int level, int accel, int prepend);

/* src/lz4.rs:88,164,168  libcramjam::lz4::block::decompress_into(in, out, Some(size_prepended))
 * size_prepended=1: u32-LE length prefix expected, decode capacity = that length;
 * size_prepended=0: raw block, decode capacity = cap.  Returns decoded byte count. */
CJ_API int64_t cj_lz4_block_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int size_prepended);

/* src/lz4.rs:90  libcramjam::lz4::block::decompress_vec reads this before allocating:
 * the u32-LE prefix, or CJ_E_NO_PREFIX when n < 4. Pure arithmetic, no device. */
CJ_API int64_t cj_lz4_block_prefixed_len(const uint8_t* in, size_t n);

/* src/snappy.rs:114  snap::raw::max_compress_len(len) = 32 + len + len/6 (0 = too big). No device. */
CJ_API size_t cj_snappy_raw_max_compress_len(size_t len);
/* src/snappy.rs:121  snap::raw::decompress_len(in): varint preamble; 0 for empty input. No device. */
CJ_API int64_t cj_snappy_raw_decompress_len(const uint8_t* in, size_t n);
/* src/snappy.rs:75,97  libcramjam::snappy::raw::compress(in, out); needs cap >= max_compress_len(n) */
CJ_API int64_t cj_snappy_raw_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* src/snappy.rs:57,106 libcramjam::snappy::raw::decompress(in, out); needs cap >= decompress_len(in) */
CJ_API int64_t cj_snappy_raw_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);

/* ---- Snappy FRAMING format: a stream of independent <= 64 KiB pieces, each with a masked
 * CRC-32C; pieces are de/compressed and checksummed on the GPU as one batch. ---- */
/* upper bound of cj_snappy_frame_compress's output: 10 + 8 * ceil(n / 65536) + n (0 for n == 0). No device. */
CJ_API size_t cj_snappy_frame_max_compress_len(size_t n);
/* src/snappy.rs:38,82  libcramjam::snappy::compress (snap read::FrameEncoder): stream identifier + one chunk per
 * 65536 input bytes, stored uncompressed when it does not shrink by 1/8; empty input -> empty output. */
CJ_API int64_t cj_snappy_frame_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* decoded length of a framed stream from its chunk headers alone (what a caller allocates before
 * cj_snappy_frame_decompress), or the first header-level error. No device. */
CJ_API int64_t cj_snappy_frame_decompress_len(const uint8_t* in, size_t n);
/* src/snappy.rs:24,88  libcramjam::snappy::decompress (snap read::FrameDecoder): errors are reported in stream
 * order like the sequential decoder would (block error, checksum, output full, then header errors).
 * out == NULL: validate only — decode and checksum on the device, return the decoded length or the first error. */
CJ_API int64_t cj_snappy_frame_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);

/* ---- LZ4 FRAME format: blocks de/compressed on the GPU — independent-block and single-block
 * frames as one batch, linked-block frames by a chain kernel; XXH32 frame checksums on a concurrent host thread. ---- */
/* upper bound of cj_lz4_frame_compress's output: 15 + 4 * ceil(n / 65536) + n. No device. */
CJ_API size_t cj_lz4_frame_compress_bound(size_t n);
/* src/lz4.rs:43,56  libcramjam::lz4::compress(input, output, level) (lz4 crate EncoderBuilder -> LZ4F): 64 KiB blocks,
 * content checksum, no content size — like the reference — but INDEPENDENT blocks (FLG 0x64; the reference links them:
 * cj_lz4_frame_compress_linked writes that frame) and one matcher for every `level` (the reference's default level 4 is
 * LZ4HC): any LZ4F decoder reads the result, and this library decodes it fastest (independent blocks are one batch). */
CJ_API int64_t cj_lz4_frame_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int level);
/* the same frame with LINKED blocks (FLG 0x44, BD 0x40; BlockMode::Linked, the reference's default): every block may refer to
 * the 64 KiB of input before it — 3.5 % fewer bytes on the reference's corpus, up to 12 % on a file.  Encoded as parallel as
 * independent blocks; decoded sequentially (this library: ~2 GB/s against 7-9 GB/s for independent blocks).  Same bound. */
CJ_API int64_t cj_lz4_frame_compress_linked(const uint8_t* in, size_t n, uint8_t* out, size_t cap, int level);
/* only the block sequence of such a frame (u32 size word + data per 64 KiB of input; no header, EndMark or checksum):
 * what a streaming encoder (reference src/lz4.rs:231-292 `Compressor`) emits per flush.  cap >= n + 4 * ceil(n / 65536). */
CJ_API int64_t cj_lz4_frame_compress_blocks(const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* the block sequence of a linked-block frame: hist = the input that precedes `in` in the frame (only its last 65536 bytes
 * count; NULL / 0 for none), what a streaming encoder passes on every flush.  Same capacity rule.  Every block is one
 * workgroup of the batch kernel, whatever n (no split pieces): its bytes are tests/hostsim/enc2_linked_model.c's. */
CJ_API int64_t cj_lz4_frame_compress_blocks_linked(const uint8_t* hist, size_t hist_len, const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* upper bound of the decoded size from the headers alone (content size if stored, else blocks x max block size), or the
 * first header-level error. No device. */
CJ_API int64_t cj_lz4_frame_decompress_bound(const uint8_t* in, size_t n);
/* src/lz4.rs:28,63  libcramjam::lz4::decompress (lz4 crate Decoder -> LZ4F_decompress): all block sizes, linked and
 * independent blocks, block / content checksums, content size; stops after the first frame like the crate's Decoder.
 * out == NULL: validate only (block structure and block decode; the content checksum needs the bytes on the host). */
CJ_API int64_t cj_lz4_frame_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);

/* =====================================================================================
 * Batch extension (no reference equivalent: the reference API is one buffer per call; a GPU only
 * pays off on batches of independent chunks).  One engine per GPU; chunks of a batch are
 * independent, so multi-GPU use is host-side round-robin sharding over engines, no collective.
 * ===================================================================================== */
typedef struct cj_engine cj_engine;

typedef enum { CJ_CODEC_LZ4_BLOCK = 0, CJ_CODEC_SNAPPY_RAW = 1 } cj_codec;
typedef enum { CJ_OP_DECOMPRESS = 0, CJ_OP_COMPRESS = 1 } cj_op;

/* flags */
#define CJ_FLAG_LZ4_SIZE_PREFIX 1u   /* lz4: blocks carry / get the u32-LE length prefix (store_size) */
/* decode mapping overrides (tests and comparisons; results are identical): one wavefront per chunk, one lane per chunk, or
 * the workgroup decoder for every chunk it can take.  Default: the workgroup decoder, the wave kernel for what it leaves over */
#define CJ_FLAG_FORCE_WAVE_PER_CHUNK 0x100u
#define CJ_FLAG_FORCE_LANE_PER_CHUNK 0x200u
#define CJ_FLAG_FORCE_LDS_PER_CHUNK  0x400u
/* ... and, for the workgroup decoder, where its parse stage runs: inside the decoder kernel / as the lane-per-chunk kernel in front of
 * it, at any batch size (default: by CJ_FUSED_MAX_CHUNKS below).  Tests exercise both sides of the threshold with them. */
#define CJ_FLAG_FORCE_FUSED_PARSE   0x10u
#define CJ_FLAG_FORCE_PARSE_KERNEL  0x20u
/* decompress, a promise about the batch: every chunk's output capacity (LZ4) / announced length (Snappy) is at most 32 KiB / 16 KiB.
 * The workgroup decoder then runs on windows of that size — four workgroups of four wavefronts / eight of two per CU instead of two of
 * eight: more chunks' dependency chains in flight for the same wavefronts (32 KiB chunks 635 -> 850 GB/s, 16 KiB 430 -> 810; batches of
 * up to CJ_FUSED_MAX_CHUNKS chunks: the one-kernel path on the same windows, 4 096 x 32 / 16 KiB 233 / 153 -> 401 / 309).  A chunk
 * that breaks the promise is still decoded correctly (one wavefront).  cj_batch_host sets them itself. */
#define CJ_FLAG_CHUNKS_LE_32K       0x40u
#define CJ_FLAG_CHUNKS_LE_16K       0x80u
/* decompress: the batch may hold chunks of 64 KiB .. 256 KiB (capacity / announced length) and they matter — the engine lists them on
 * the device, parses them with 32 lanes each into record areas (1 MiB per listed chunk, groups of up to 8 192) and decodes them slab by
 * slab with workgroups.  How many there are is known on the device only: every flagged call copies its count back
 * WITHOUT waiting for it, and a call reserves for the largest of the last eight counts that have arrived; what a batch holds beyond
 * that — and every such chunk without the flag — takes one wavefront: correct, ~2.5x slower in bulk.  Only the first flagged call
 * on an engine waits for the stream once (it reads its own count); like every call, one that has to GROW the engine's scratch waits
 * for the device while it reallocates.  After that cj_batch_device with this flag only enqueues. */
#define CJ_FLAG_BIG_CHUNKS          0x800u
/* debug aid: the workgroup decoder accumulates per-phase cycle counters (read with cj_debug_lds_phase_cycles, cramjam_hip_debug.h; results unchanged) */
#define CJ_FLAG_DEBUG_PROFILE        0x1000u
/* decode batches up to this many chunks run parse + decode as ONE kernel (the segmented parse inside the workgroup decoder:
 * 1 chunk 0.16 ms instead of 0.25, 8 192 chunks 348 instead of 178 GB/s); above, a lane-per-chunk parse kernel in front of the
 * decoder is cheaper per chunk.  The crossover depends on the data — the parse kernel's fixed latency is one lane walking one
 * chunk, i.e. its sequence count: benchmark data (2.7 k sequences per 64 KiB) ~13 000 chunks for LZ4 and ~10 500 for Snappy,
 * the reference's corpus (~8 k) above 24 000 (profiles/r04/experiments, c02); 16 384 loses at most ~11 % on either side */
#define CJ_FUSED_MAX_CHUNKS 16384
/* decode batches larger than this are submitted in slices of this many chunks */
#define CJ_SLICE_CHUNKS_DEFAULT 131072

CJ_API int  cj_engine_create(int device, cj_engine** out);
CJ_API void cj_engine_destroy(cj_engine* e);
CJ_API int  cj_engine_device(const cj_engine* e);

/* Device-resident batch: every pointer is a DEVICE pointer on the engine's GPU.
 * chunk i reads  in_base + in_off[i] .. + in_len[i]   and writes  out_base + out_off[i] .. + out_cap[i];
 * in_off / out_off are full 64-bit byte offsets: a batch may span more than 4 GiB, and a chunk may lie across a 4 GiB boundary.
 * result[i] = bytes produced (>= 0) or CJ_E_* (< 0); one bad chunk never affects another.
 * hip_stream: a hipStream_t (NULL = the engine's own stream).  Asynchronous: returns after enqueue;
 * call cj_engine_sync (or synchronise the stream yourself) before reading results.
 * Input addressing: chunks may start at any byte alignment, but the kernels fetch the stream with aligned vector loads —
 * the 16-byte granules that hold a chunk's first and last byte are read whole (up to 15 bytes before in_base + in_off[i]
 * and up to 15 bytes past its end; never used, never written).  Both granules must therefore lie inside the device
 * allocation: true for every chunk of a buffer that comes from hipMalloc / a caching allocator (allocations start on
 * 256-byte boundaries and are padded to their granule), NOT for a chunk that begins or ends flush with a page the
 * caller carved up itself.  cj_batch_host pads to 16 bytes on its own staging buffers. */
CJ_API int cj_batch_device(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                    const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                    uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                    int64_t* result, void* hip_stream);
CJ_API int cj_engine_sync(cj_engine* e);
/* the same for a caller's stream (a hipStream_t; NULL = the engine's own): what a binding without its own HIP runtime handle needs
 * to wait for a batch it submitted on a stream it was handed (cramjam_amd.batch.*_device(stream=...)) */
CJ_API int cj_stream_sync(cj_engine* e, void* hip_stream);

/* Host batch: host pointers; the engine packs inputs into pinned staging, copies H2D, runs the
 * kernels, copies D2H and scatters — a batch of 128 MiB and more in slices of ~64 MiB, so that those
 * steps overlap (same results as one pass).  Synchronous. result[i] as above. */
CJ_API int cj_batch_host(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                  const uint8_t* const* in_ptrs, const size_t* in_lens,
                  uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);

/* Timing aid for benchmarks: runs the same device batch `reps` times on the engine stream between
 * two hipEvents and returns the mean kernel time per rep in milliseconds (< 0 on error). */
CJ_API double cj_batch_device_timed(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                             const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                             uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                             int64_t* result, int reps);

/* Batches of framed streams: LZ4 frames (cj_lz4_frame_*) or Snappy framed streams (cj_snappy_frame_*), one independent stream
 * per entry.  Addressing, alignment and stream rules are cj_batch_device's: stream i reads in_base + in_off[i] .. + in_len[i] and
 * writes only inside out_base + out_off[i] .. + out_cap[i].  flags is reserved (0); an unknown fmt or op is CJ_E_BAD_ARG.
 *   decompress  result[i] = what cj_lz4_frame_decompress / cj_snappy_frame_decompress return for stream i alone with cap = out_cap[i]
 *               (the same error, by the same stream-order precedence), and the same bytes when >= 0.
 *   compress    result[i] = frame size or CJ_E_* (CJ_E_FRAME_WRITE when out_cap[i] is too small; nothing is written then).  The
 *               single-call layout (LZ4: FLG 0x64 / BD 0x40, 64 KiB independent blocks, content checksum; Snappy: stream identifier,
 *               64 KiB chunks, masked CRC-32C) with the payloads of cj_batch_device's compress of each 64 KiB piece.
 * Everything specific to the format runs on the device (grammar walk, XXH32, CRC-32C, verdicts, assembly).  NOT enqueue-only: the
 * device call waits for hip_stream once — it reads back the streams' block counts (decompress) / in_len (compress) to size the
 * block table and the grids — then enqueues the rest and returns; synchronise before reading result.  The host call is pack ->
 * H2D -> the device path -> D2H -> scatter, synchronous.  Frame batches on one engine run one after another (a call holds the engine's
 * frame-batch scratch across its wait, so a second caller also waits behind what the first queued on its stream). */
typedef enum { CJ_FORMAT_LZ4_FRAME = 0, CJ_FORMAT_SNAPPY_FRAMED = 1 } cj_format;
CJ_API int cj_frame_batch_device(cj_engine* e, cj_format fmt, cj_op op, uint32_t flags, size_t n_frames,
                                 const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                 uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                 int64_t* result, void* hip_stream);
CJ_API int cj_frame_batch_host(cj_engine* e, cj_format fmt, cj_op op, uint32_t flags, size_t n_frames,
                               const uint8_t* const* in_ptrs, const size_t* in_lens,
                               uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);

/* Decoded-size queries: what a caller needs to lay out out_off / out_cap before it can submit cj_batch_device / cj_frame_batch_device,
 * for chunks that may live in device memory only.  result[i] = the decoded size of chunk i (>= 0) or CJ_E_* (< 0); nothing but result
 * is written.  Addressing, alignment (the 16-byte granules of a chunk's first and last byte may be read whole), stream and thread
 * safety are cj_batch_device's.  The _device calls are ENQUEUE-ONLY: no wait on the stream, no read-back, no engine scratch, no lock
 * — a query may sit in front of a decode on the same stream (compute the capacities from result on the device), and it does not wait
 * behind a frame batch that runs on another stream of the same engine.  The _host calls are pack -> H2D -> the device path -> D2H of
 * the results, synchronous.  n == 0 succeeds; a null pointer with n > 0, an unknown codec / fmt, or a flag bit other than
 * CJ_FLAG_LZ4_SIZE_PREFIX (frames: any bit) is CJ_E_BAD_ARG.  e == NULL: the default engine of device 0; without a usable device
 * CJ_E_NO_DEVICE.
 *   Snappy raw          cj_snappy_raw_decompress_len of the chunk: the announced length or its header error, 0 for an empty chunk.
 *                       Header only (the reference's decompress_raw_len): a later decode may still fail.
 *   LZ4 block, CJ_FLAG_LZ4_SIZE_PREFIX   the u32 prefix, by the decoder's rules that need no capacity: CJ_E_NO_PREFIX, CJ_E_NEG_PREFIX,
 *                       CJ_E_PREFIX_TOO_BIG (and CJ_E_CORRUPT for more than 0x7FFFFFF0 bytes behind the prefix).  Header only.
 *   LZ4 block, raw      the WALK: the length S the safe decoder produces when output room never runs out (LZ4_decompress_safe with a
 *                       capacity of 255 * in_len + 64, the rule cj_lz4_frame_decompress_bound relies on).  CJ_E_CORRUPT where that
 *                       decode fails: malformed length fields, input not consumed exactly, offset 0 (this library rejects it), an
 *                       offset beyond the bytes produced so far, an empty chunk, in_len > 0x7FFFFFF0.  CJ_E_PREFIX_TOO_BIG when
 *                       S > 0x7E000000: no capacity the decoder accepts can hold it.  The match bytes are not looked at: S is exact.
 *                       Contract with cj_batch_device (decompress, no prefix): with out_cap[i] >= S + CJ_LZ4_SIZE_SLACK every chunk
 *                       the query accepted decodes to exactly S bytes; with out_cap[i] == S it does whenever the block obeys LZ4's
 *                       end-of-block rules (the last sequence is literals only, the last match ends 5 bytes before the end and starts
 *                       12 before it: every encoder's output does).  The slack is not a measurement: the decoder asks a non-final
 *                       sequence for cap - op >= literals + 12 and, behind its literals, for cap - op >= match + 5; with
 *                       cap = S + 12 both hold for every sequence of a stream whose total is S.
 *                       Chunks of up to 64 KiB of data are the fast case (one lane each); a longer chunk takes one wavefront.
 *   LZ4 frame           cj_lz4_frame_decompress_bound of the frame: an upper bound by that function's rules, 0 for a skippable frame
 *   Snappy framed       cj_snappy_frame_decompress_len of the stream */
#define CJ_LZ4_SIZE_SLACK 12
CJ_API int cj_batch_sizes_device(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks,
                                 const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                 int64_t* result, void* hip_stream);
CJ_API int cj_batch_sizes_host(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks,
                               const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);
CJ_API int cj_frame_batch_sizes_device(cj_engine* e, cj_format fmt, uint32_t flags, size_t n_frames,
                                       const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                       int64_t* result, void* hip_stream);
CJ_API int cj_frame_batch_sizes_host(cj_engine* e, cj_format fmt, uint32_t flags, size_t n_frames,
                                     const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);

/* Batches of LZ4 blocks against ONE dictionary shared by every chunk of the call: the blocks LZ4_loadDict + LZ4_compress_fast_continue
 * write and LZ4_decompress_safe_usingDict reads (the block stores of small records: RocksDB-style blocks, message logs, column pages).
 * Arguments, addressing, alignment, result[i] and stream rules are cj_batch_device's / cj_batch_host's / the size queries'; the
 * dictionary (dict_dev: device memory, dict_host: host memory, uploaded once per call) is borrowed for the call.  Only its last
 * 65 536 bytes count, as in liblz4; dict_len == 0 IS the plain call (cj_batch_device, cj_batch_host, cj_batch_sizes_*), result for
 * result and byte for byte.  e == NULL: the default engine of device 0.
 *   codec       CJ_CODEC_LZ4_BLOCK.  Snappy has no dictionaries: CJ_E_BAD_ARG.
 *   flags       0 or CJ_FLAG_LZ4_SIZE_PREFIX.  Every other bit — the mapping overrides included — is REFUSED with CJ_E_BAD_ARG: a
 *               dictionary batch has one mapping (one wavefront per chunk; the workgroup decoders hold no dictionary window).
 *   decompress  lz4_wave_decode's rules; a match of `offset` > the bytes produced so far begins offset - produced bytes before the
 *               dictionary's end.  CJ_E_CORRUPT: offset 0, or offset > produced + min(dict_len, 65536).  Chunks of any size.
 *   sizes       the walk of cj_batch_sizes_device with that offset rule: it needs dict_len only, not the bytes.  Same contract with the
 *               decode (CJ_LZ4_SIZE_SLACK).  With CJ_FLAG_LZ4_SIZE_PREFIX: the prefix, as without a dictionary.
 *   compress    chunks of at most 65 536 bytes; a longer one gets CJ_E_INPUT_TOO_LARGE in its own result[i].  Capacities as for
 *               cj_batch_device (cj_lz4_block_compress_bound).  The engine stages `dictionary tail | chunk` per chunk in its scratch (in
 *               slices of at most 1 GiB) and runs the linked-block encoder of cj_lz4_frame_compress_linked over it: every chunk indexes
 *               the dictionary again, a pass over n x (min(dict_len, 65536) + chunk) bytes.
 *   a null dict with dict_len > 0, an unknown op, a null batch pointer with n_chunks > 0: CJ_E_BAD_ARG.  n_chunks == 0 succeeds.
 * The _device calls only enqueue (like every call, one that has to GROW the engine's scratch — compress — waits for its previous user
 * while it reallocates).  The _host calls are cj_batch_host's one-shot staging, synchronous. */
CJ_API int cj_dict_batch_device(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                                const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                int64_t* result, const uint8_t* dict_dev, size_t dict_len, void* hip_stream);
CJ_API int cj_dict_batch_host(cj_engine* e, cj_codec codec, cj_op op, uint32_t flags, size_t n_chunks,
                              const uint8_t* const* in_ptrs, const size_t* in_lens,
                              uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result,
                              const uint8_t* dict_host, size_t dict_len);
CJ_API int cj_dict_batch_sizes_device(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks,
                                      const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                      int64_t* result, size_t dict_len, void* hip_stream);
CJ_API int cj_dict_batch_sizes_host(cj_engine* e, cj_codec codec, uint32_t flags, size_t n_chunks,
                                    const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result, size_t dict_len);

/* Batches of DEFLATE streams — decode only: raw DEFLATE (RFC 1951: ORC's zlib codec), zlib streams (RFC 1950: Zarr / numcodecs Zlib)
 * and gzip members (RFC 1952: Parquet GZIP pages, numcodecs GZip).  One chunk is exactly ONE stream, one wavefront decodes it
 * (DESIGN.md 5.12); the accept / reject rules are zlib's inflate.  Addressing, the 16-byte-granule rule, stream rules, e == NULL,
 * n_chunks == 0 and the null-pointer rules are cj_batch_device's / cj_batch_host's / cj_batch_sizes_*'s.
 *   wrap        a cj_deflate_wrap; anything else is CJ_E_BAD_ARG.
 *   op          CJ_OP_DECOMPRESS.  CJ_OP_COMPRESS and any other value: CJ_E_BAD_ARG — the encoder has entry points of its own
 *               (cj_deflate_compress_batch_*, below).
 *   flags       0.  Any bit set is CJ_E_BAD_ARG.
 *   result[i]   the decoded length (>= 0) or CJ_E_*; one bad chunk never affects another; nothing is written outside
 *               out_base + out_off[i] .. + out_cap[i], and what lies behind result[i] bytes (or anywhere in the slot of a chunk with an
 *               error) is unspecified.  in_len[i] > 0x7FFFFFF0 is CJ_E_CORRUPT, out_cap[i] > 0x7E000000 is CJ_E_PREFIX_TOO_BIG, in that
 *               chunk's own result[i], as elsewhere in this library.
 *   errors      the FIRST one in stream order.  CJ_E_DEFLATE_HEADER: zlib — CM != 8, CINFO > 7, a bad FCHECK, FDICT (preset dictionaries
 *               are not supported); gzip — a bad magic, CM != 8, a reserved FLG bit, a bad FHCRC (FEXTRA, FNAME, FCOMMENT and FHCRC are
 *               walked).  CJ_E_DEFLATE_CORRUPT: block type 3, stored LEN / ~LEN mismatch, more than 286 length or 30 distance symbols, a
 *               bad code-length repeat, an over-subscribed code, an incomplete code where zlib refuses it (all but a single code of
 *               length 1 in a data alphabet), no end-of-block code, literal/length symbols 286 / 287, distance symbols 30 / 31, a
 *               distance beyond the bytes produced so far.  A symbol's own validity comes before its fit: a match with a bad distance
 *               that would also overrun the capacity is CJ_E_DEFLATE_CORRUPT.  CJ_E_OUT_TOO_SMALL: raised before the first byte that
 *               would not fit is written.  CJ_E_DEFLATE_EOF: the input ends before the final block's end-of-block code or inside the
 *               trailer.  CJ_E_DEFLATE_CHECKSUM: Adler-32 (zlib), CRC-32 or ISIZE (gzip), compared only after the stream has ended well.
 *               CJ_E_DEFLATE_TRAILING: raw — whole bytes behind the byte that holds the final block's last bit; zlib / gzip — anything
 *               behind the trailer.  A second gzip member IS trailing data: multi-member gzip files are split by the caller.
 *   sizes       the same decoder with its stores and checksums compiled out: result[i] = the exact decoded length of a stream that is
 *               valid up to its end, with the decoder's header, data, EOF and trailing errors; a total above 0x7E000000 is
 *               CJ_E_PREFIX_TOO_BIG.  The checksums are NOT verified by the size query (it writes no output to sum), and gzip's ISIZE is
 *               neither trusted nor read for the size: a stream the query sizes can still be CJ_E_DEFLATE_CHECKSUM in the decode.
 * The _device calls only enqueue: no wait, no read-back, no engine scratch, no lock.  The _host calls are cj_batch_host's one-shot
 * staging, synchronous. */
typedef enum { CJ_DEFLATE_RAW = 0, CJ_DEFLATE_ZLIB = 1, CJ_DEFLATE_GZIP = 2 } cj_deflate_wrap;
CJ_API int cj_deflate_batch_device(cj_engine* e, cj_deflate_wrap wrap, cj_op op, uint32_t flags, size_t n_chunks,
                                   const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                   uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                   int64_t* result, void* hip_stream);
CJ_API int cj_deflate_batch_host(cj_engine* e, cj_deflate_wrap wrap, cj_op op, uint32_t flags, size_t n_chunks,
                                 const uint8_t* const* in_ptrs, const size_t* in_lens,
                                 uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API int cj_deflate_batch_sizes_device(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks,
                                         const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                         int64_t* result, void* hip_stream);
CJ_API int cj_deflate_batch_sizes_host(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks,
                                       const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);

/* Batches of inputs INTO DEFLATE streams: one chunk in gives exactly one stream out — raw: RFC 1951 blocks, BFINAL on
 * the last one only, the unused bits of the last byte 0; zlib: 78 01, the blocks, Adler-32 big-endian; gzip: a fixed 10-byte header (no
 * flags, MTIME 0, XFL 0, OS 255), the blocks, CRC-32 and ISIZE.  The bytes depend on nothing but the input and the wrapper; an empty
 * input gives a valid stream of one final block.  The input is cut into independent pieces of at most 64 KiB (no match crosses a
 * piece, distances up to 32 768), each piece one block — stored, fixed or dynamic, whichever is smallest — behind the bit position the
 * previous block left.  What cj_deflate_batch_* (zlib's inflate) accepts is the contract.  Addressing, the 16-byte-granule rule,
 * stream rules, e == NULL, n_chunks == 0 and the null-pointer rules are cj_deflate_batch_*'s.
 *   wrap        a cj_deflate_wrap; anything else is CJ_E_BAD_ARG.      flags   0; any bit set is CJ_E_BAD_ARG.
 *   result[i]   the stream's length or CJ_E_*: in_len[i] > 0x7E000000 is CJ_E_INPUT_TOO_LARGE in that chunk's own result;
 *               CJ_E_OUT_TOO_SMALL when the stream does not fit out_cap[i] (checked per block from its exact cost, before its first
 *               store: nothing is written at or behind out_cap[i]; what lies in the slot of such a chunk is unspecified).
 *   bound       cj_deflate_compress_bound(n, wrap): the exact worst case of this layout (every piece stored, two stored blocks for a
 *               full piece, each header spilling into a byte of its own) = n + 10 * (n / 65536) + 5 * (n % 65536 != 0 || n == 0) +
 *               0 / 6 / 18 for raw / zlib / gzip; a capacity of that many bytes never gives CJ_E_OUT_TOO_SMALL.  0 for a bad wrap or
 *               n > 0x7E000000.  Pure arithmetic, no device.
 * The _device call only enqueues (like every call, one that has to GROW the engine's scratch — the workgroups' record slots, within a
 * fixed budget — waits for its previous user while it reallocates).  The _host call is cj_batch_host's one-shot staging, synchronous. */
CJ_API int cj_deflate_compress_batch_device(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks,
                                            const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                            uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                            int64_t* result, void* hip_stream);
CJ_API int cj_deflate_compress_batch_host(cj_engine* e, cj_deflate_wrap wrap, uint32_t flags, size_t n_chunks,
                                          const uint8_t* const* in_ptrs, const size_t* in_lens,
                                          uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API size_t cj_deflate_compress_bound(size_t n, cj_deflate_wrap wrap);

/* Batches of BGZF streams, both directions: the blocked gzip of the SAM specification (4.1) — BAM, BCF, tabix-indexed
 * VCF, every `bgzip` file.  A stream is zero or more RFC 1952 gzip members of at most 64 KiB laid end to end with nothing between or
 * behind them; each has FEXTRA set and, among its extra subfields, one `BC` subfield of two bytes: BSIZE, the member's length - 1 (the
 * first one counts; other subfields, FNAME, FCOMMENT and FHCRC are walked).  The members are found without decoding, so one entry of
 * these batches is a whole stream of any size and every member of every stream is decoded (encoded) by a wavefront (workgroup) of its
 * own.  The end-of-file marker, an empty member of 28 bytes, is not required and decodes to nothing, like an empty member anywhere.
 * The argument shape is cj_frame_batch_*'s; addressing, the 16-byte-granule rule, stream rules, e == NULL, n_streams == 0 and the
 * null-pointer rules are cj_deflate_batch_*'s.
 *   what        0; anything else is CJ_E_BAD_ARG.      flags   0; any bit set is CJ_E_BAD_ARG.
 *   op          CJ_OP_DECOMPRESS or CJ_OP_COMPRESS; anything else is CJ_E_BAD_ARG.  These checks come first and need no device.
 *   decompress  result[i] = the decoded length, the sum of the members' ISIZE, or CJ_E_*.  The walk's errors come first, at the first
 *               member in stream order that has one: CJ_E_DEFLATE_EOF — fewer than 12 bytes, or than 12 + XLEN, are left, or the
 *               member runs past the input's end; CJ_E_DEFLATE_HEADER — a bad magic, CM != 8, FEXTRA clear, a subfield that runs
 *               past XLEN, no BC subfield of two bytes, a BSIZE without room for an empty block and the trailer.  Bytes behind the
 *               last member fail these checks: zero padding, which other gzip readers tolerate, is an error here.  Then
 *               CJ_E_OUT_TOO_SMALL when the ISIZE sum exceeds out_cap[i].  A stream refused so far is not decoded and its slot is not
 *               written.  Every member then decodes into its own ISIZE bytes of the slot, behind those of the members before it, by
 *               cj_deflate_batch_*'s rules for CJ_DEFLATE_GZIP; the stream's result is the code of the first failing member in stream
 *               order, a member that holds more than its ISIZE says being CJ_E_DEFLATE_CHECKSUM (zlib's "incorrect length check").
 *               A stream with a bad member may have written inside its own slot, never outside it; one bad stream never affects
 *               another.
 *   sizes       cj_bgzf_sizes_*: the walk alone — result[i] = the ISIZE sum or the walk's error.  The sizes are CLAIMS read from the
 *               members' trailers: only the decode verifies them (and the checksums).
 *   compress    one stream per buffer: members of 65 280 input bytes (htslib's block size), the last one shorter, then the marker;
 *               an empty buffer gives the marker alone.  A member is the 18-byte header 1f 8b 08 04, MTIME 0, XFL 0, OS 255, XLEN 6,
 *               `BC` 2 0 BSIZE, then exactly the DEFLATE block, CRC-32 and ISIZE that cj_deflate_compress_batch_* writes for that
 *               piece.  The bytes depend on nothing but the input.  result[i] = the stream's length; CJ_E_INPUT_TOO_LARGE for
 *               in_len[i] > 0x7E000000; CJ_E_OUT_TOO_SMALL when the stream does not fit out_cap[i] — decided before the first store:
 *               a stream that fails writes nothing.
 *   bound       cj_bgzf_compress_bound(n): the members' worst cases (65 311 bytes for a full one, r + 31 for a last one of r bytes)
 *               plus the marker's 28; a capacity of that many bytes never gives CJ_E_OUT_TOO_SMALL.  0 for n > 0x7E000000.  Pure
 *               arithmetic, no device.
 * The batch calls take one turn at the engine's container scratch and wait for the stream ONCE (decompress: for the streams' member
 * counts; compress: for the buffers' lengths and capacities), like cj_frame_batch_*; the member encoder's slots are engine scratch
 * within a fixed budget, a large batch runs in turns.  The size query only enqueues.  The _host calls are cj_batch_host's one-shot
 * staging, synchronous. */
CJ_API int cj_bgzf_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_streams,
                                const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                int64_t* result, void* hip_stream);
CJ_API int cj_bgzf_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_streams,
                              const uint8_t* const* in_ptrs, const size_t* in_lens,
                              uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API int cj_bgzf_sizes_device(cj_engine* e, int what, uint32_t flags, size_t n_streams,
                                const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                int64_t* result, void* hip_stream);
CJ_API int cj_bgzf_sizes_host(cj_engine* e, int what, uint32_t flags, size_t n_streams,
                              const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);
CJ_API size_t cj_bgzf_compress_bound(size_t n);

/* Batches of ORC compression streams, both directions: the framing of every data stream, index stream, stripe footer
 * and file footer of an ORC file with compression != NONE (ORC specification, "Compression").  A stream is zero or more chunks; a chunk
 * is a 3-byte little-endian header h and h >> 1 bytes: with h & 1 the original bytes, else the codec's output for at most block_size
 * (the file's compressionBlockSize) raw bytes.  Nothing states a chunk's decoded length; there is no magic, no checksum and no end
 * marker.  One entry of these batches is a whole stream of any size; every chunk of every stream is decoded (encoded) by the codec's
 * plain batch.  Finding the streams in a file (the protobuf footers) is the reader's.  The argument shape is cj_bgzf_batch_*'s with
 * block_size behind flags; addressing, the 16-byte-granule rule, stream rules, e == NULL, n_streams == 0 and the null-pointer rules are
 * cj_deflate_batch_*'s.
 *   what        ORC's CompressionKind: 1 ZLIB (raw DEFLATE, no zlib header), 2 SNAPPY (Snappy raw with its varint length), 4 LZ4 (a
 *               raw LZ4 block, no size prefix), 5 ZSTD (one Zstandard frame).  Anything else (NONE 0, LZO 3, BROTLI 6) is CJ_E_BAD_ARG.
 *   flags       0; any bit set is CJ_E_BAD_ARG.       op   CJ_OP_DECOMPRESS or CJ_OP_COMPRESS; anything else is CJ_E_BAD_ARG.
 *   block_size  1 .. 2^23 for decompress and sizes (a header's length field has 23 bits), 1 .. 262 144 for compress; outside these
 *               CJ_E_BAD_ARG.  These checks come first and need no device.
 *   decompress  result[i] = the decoded length or CJ_E_*.  First the walk over the headers: CJ_E_ORC_HEADER — fewer than 3 bytes are
 *               left where a header must stand, or a chunk's length runs past the stream's end.  Then the sizes of the chunks — an
 *               original chunk's length, a compressed chunk's by the codec's size query (cj_deflate_batch_sizes_* for CJ_DEFLATE_RAW,
 *               cj_batch_sizes_* for raw LZ4 blocks and Snappy raw, cj_zstd_batch_sizes_*): the first chunk in stream order whose
 *               size is an error, or above block_size (CJ_E_ORC_BLOCK), gives its code.  Then CJ_E_OUT_TOO_SMALL when the sizes' sum
 *               exceeds out_cap[i].  A stream refused so far is not decoded and its slot is not written.  Every chunk then decodes
 *               (is copied) into its own bytes of the slot, behind those of the chunks before it; the stream's result is the code of
 *               the first chunk in stream order whose decode does not give exactly its size — a Snappy header that lies gives
 *               CJ_E_SNAPPY_CORRUPT.  A stream with a bad chunk may have written inside its own slot, never outside it; one bad stream
 *               never affects another.
 *   sizes       cj_orc_sizes_*: the same up to the sum — result[i] = the decoded length or the first error.  For ZLIB, LZ4 and ZSTD
 *               the size query walks every chunk's stream to its end; for SNAPPY the length is the header's claim, which only the
 *               decode verifies.
 *   compress    one stream per buffer: pieces of block_size bytes, the last one shorter, each through the codec's plain encoder
 *               (cj_deflate_compress_batch_* with CJ_DEFLATE_RAW, cj_batch_device for LZ4 without prefix and Snappy raw,
 *               cj_zstd_compress_batch_* without checksum); a piece whose compressed length is not below its raw length becomes an
 *               original chunk.  An empty buffer gives an empty stream (result 0).  The bytes depend on nothing but the input.
 *               result[i] = the stream's length; CJ_E_INPUT_TOO_LARGE for in_len[i] > 0x7E000000; CJ_E_OUT_TOO_SMALL when out_cap[i]
 *               is below cj_orc_compress_bound(in_len[i], block_size) — decided before the first store: such a stream writes nothing.
 *   bound       cj_orc_compress_bound(n, block_size) = n + 3 * ceil(n / block_size): every piece an original chunk; exact for
 *               incompressible input, 0 for n == 0.  Also 0 for n > 0x7E000000 or a block_size compress does not take.  Pure
 *               arithmetic, no device.
 * NONE of these calls is enqueue-only, the size query included: each takes one turn at the engine's container scratch and waits for
 * the stream ONCE (decompress, sizes: for the streams' chunk counts; compress: for the buffers' lengths and capacities); the encoder's
 * bound-sized chunk slots are engine scratch within a fixed budget, a large batch runs in turns.  The _host calls are cj_batch_host's
 * one-shot staging, synchronous. */
CJ_API int cj_orc_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, uint32_t block_size, size_t n_streams,
                               const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                               uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                               int64_t* result, void* hip_stream);
CJ_API int cj_orc_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, uint32_t block_size, size_t n_streams,
                             const uint8_t* const* in_ptrs, const size_t* in_lens,
                             uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API int cj_orc_sizes_device(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n_streams,
                               const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                               int64_t* result, void* hip_stream);
CJ_API int cj_orc_sizes_host(cj_engine* e, int what, uint32_t flags, uint32_t block_size, size_t n_streams,
                             const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);
CJ_API size_t cj_orc_compress_bound(size_t n, uint32_t block_size);

/* Batches of Parquet column chunks, decode only: the page walk, the page bodies' codecs and the page CRCs.  One entry
 * is a column chunk as it lies in the file — total_compressed_size bytes from dictionary_page_offset (data_page_offset where the
 * chunk has no dictionary page): a run of pages that tile it exactly, each a Thrift compact PageHeader and compressed_page_size bytes.
 * A DATA_PAGE_V2 puts its repetition and its definition levels, uncompressed, in front of the values; both stated sizes include them,
 * and the codec applies to the values only, and only if the header's is_compressed (default true) says so.  The decoded chunk is the
 * pages' decoded bytes one after another (V2: levels, then the decoded values).  Finding the chunks (the footer), and decoding levels
 * and values (PLAIN, RLE_DICTIONARY, ...), are the reader's.  The footer's total_uncompressed_size counts the header bytes too: it is
 * an upper bound on the decoded length and always suffices as a capacity.  The argument shape is cj_bgzf_batch_*'s; addressing, the
 * 16-byte-granule rule, stream rules, e == NULL, n_chunks == 0 and the null-pointer rules are cj_deflate_batch_*'s.
 *   what        Parquet's CompressionCodec: 0 UNCOMPRESSED (every page is copied), 1 SNAPPY (Snappy raw), 2 GZIP (one gzip member per
 *               page), 6 ZSTD (one frame), 7 LZ4_RAW (a raw LZ4 block).  Anything else — LZO 3, BROTLI 4, the deprecated
 *               Hadoop-framed LZ4 5 — is CJ_E_BAD_ARG.
 *   op          CJ_OP_DECOMPRESS; anything else is CJ_E_BAD_ARG.
 *   flags       0 or CJ_PARQUET_FLAG_VERIFY_CRC (the batch calls only; sizes and pages take 0); any other bit is CJ_E_BAD_ARG.  These
 *               checks come first and need no device.
 *   headers     the compact protocol as parquet_grammar.hpp states it: unknown field ids (Statistics among them) are skipped by their
 *               type through at most 8 containers inside one another; a known id must have its type; of a known id that appears
 *               twice the last one counts; an I32 is the low 32 bits of its zigzag varint.  PageHeader: 1 type, 2
 *               uncompressed_page_size, 3 compressed_page_size (all three required), 4 crc, 5 DataPageHeader (num_values, encoding and
 *               the two level encodings required), 7 DictionaryPageHeader (num_values, encoding), 8 DataPageHeaderV2 (fields 1 - 6
 *               required).  Page types 0, 2 and 3 must carry their own struct.  A page of any other type is listed and skipped: it
 *               adds nothing to the decoded chunk, and its payload is neither decoded nor checksummed.
 *   decompress  result[i] = the decoded length, the sum of the read pages' uncompressed_page_size, or CJ_E_*.  First the walk over
 *               the headers: CJ_E_PARQUET_HEADER at the first page that has it.  Then CJ_E_OUT_TOO_SMALL when the sum exceeds
 *               out_cap[i].  A chunk refused so far is not decoded and its slot is not written.  Every page then decodes (is copied)
 *               into its own bytes of the slot, behind those of the pages before it; the chunk's result is the code of the first page
 *               in page order that has one: CJ_E_PARQUET_CRC (with CJ_PARQUET_FLAG_VERIFY_CRC, a page whose header carries a crc:
 *               the CRC-32, gzip's, of the whole payload as it lies in the file, levels included); else the decoder's code
 *               (cj_batch_device for Snappy raw and raw LZ4 blocks, cj_deflate_batch_* with CJ_DEFLATE_GZIP, cj_zstd_batch_*, each
 *               with the stated size of the values as the capacity); else CJ_E_PARQUET_SIZE when the stream ended well with fewer
 *               bytes than stated.  Decoding is not gated on the CRC.  A values section of 0 bytes that states 0 bytes is accepted
 *               without asking the codec.  A page that is copied — every page of an UNCOMPRESSED chunk, a V2 page with is_compressed
 *               false — is not checked for size: min(compressed_page_size, uncompressed_page_size) bytes are copied.  A chunk with a
 *               bad page may have written inside its own slot, never outside it; one bad chunk never affects another.
 *   sizes       cj_parquet_sizes_*: the walk alone — result[i] = the sum or CJ_E_PARQUET_HEADER.  The sizes are the headers' claims,
 *               verified only by the decode.  ENQUEUE-ONLY: no wait, no read-back, no engine scratch.
 *   pages       cj_parquet_pages_*: the walk's page table, what a device-resident reader needs to make sense of the decoded chunk.
 *               rows == NULL: result[i] = the page count or CJ_E_PARQUET_HEADER.  Otherwise eight int64 per page are written at
 *               rows + 8 * row_off[i] (host: at rows_ptrs[i]) and result[i] = the page count; more pages than row_cap[i] is
 *               CJ_E_OUT_TOO_SMALL, and like a chunk with CJ_E_PARQUET_HEADER it writes nothing.  The words: 0 page type; 1 payload
 *               offset in the chunk; 2 compressed_page_size; 3 uncompressed_page_size; 4 offset in the decoded chunk (a skipped page
 *               takes no room there: the next page has the same offset); 5 num_values | num_rows << 32 (num_rows 0 outside V2); 6
 *               encoding | definition_level_encoding << 8 | repetition_level_encoding << 16 | is_compressed << 24 | has_crc << 25; 7
 *               definition_levels_byte_length | repetition_levels_byte_length << 32.  flags 0.  ENQUEUE-ONLY like the size query.
 * cj_parquet_batch_device takes one turn at the engine's container scratch and waits for the stream ONCE, for the chunks' page counts
 * and largest page (from which it picks CJ_FLAG_CHUNKS_LE_16K / _32K / CJ_FLAG_BIG_CHUNKS for Snappy and LZ4); the headers state every
 * decoded size, so nothing is walked twice by a codec.  The _host calls are cj_batch_host's one-shot staging, synchronous.
 * Not read: multi-member gzip pages (CJ_E_DEFLATE_TRAILING), page indexes, bloom filters, encrypted files. */
#define CJ_PARQUET_FLAG_VERIFY_CRC 1u
CJ_API int cj_parquet_batch_device(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_chunks,
                                   const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                   uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                   int64_t* result, void* hip_stream);
CJ_API int cj_parquet_batch_host(cj_engine* e, int what, cj_op op, uint32_t flags, size_t n_chunks,
                                 const uint8_t* const* in_ptrs, const size_t* in_lens,
                                 uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API int cj_parquet_sizes_device(cj_engine* e, int what, uint32_t flags, size_t n_chunks,
                                   const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                   int64_t* result, void* hip_stream);
CJ_API int cj_parquet_sizes_host(cj_engine* e, int what, uint32_t flags, size_t n_chunks,
                                 const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);
CJ_API int cj_parquet_pages_device(cj_engine* e, uint32_t flags, size_t n_chunks,
                                   const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                   int64_t* rows, const uint64_t* row_off, const uint64_t* row_cap,
                                   int64_t* result, void* hip_stream);
CJ_API int cj_parquet_pages_host(cj_engine* e, uint32_t flags, size_t n_chunks,
                                 const uint8_t* const* in_ptrs, const size_t* in_lens,
                                 int64_t* const* rows_ptrs, const size_t* row_caps, int64_t* result);

/* Batches of decoded Parquet column chunks INTO column chunks: the writer beside cj_parquet_batch_*.  The caller has
 * the pages' DECODED bytes one after another (V2: repetition levels, definition levels, values) — exactly what cj_parquet_batch_*
 * writes — and the chunk's page table in the layout of cj_parquet_pages_*, so a decoded chunk's table can be passed straight back
 * (Parquet-to-Parquet recompression: decode, pages, compress with another codec).  Everything else runs on the device in one call: the
 * codec over every values section, per V2 page whether compression paid, the CRC-32 of every payload, the Thrift compact PageHeaders,
 * the layout and the assembly.  Addressing, the 16-byte-granule rule, stream rules, e == NULL, n_chunks == 0 and the null-pointer
 * rules are cj_parquet_batch_*'s (rows, row_off and row_cnt count among the rows that must be present).
 *   what        Parquet's CompressionCodec as cj_parquet_batch_* takes it: 0, 1, 2, 6, 7; anything else is CJ_E_BAD_ARG.
 *   flags       0; any bit set is CJ_E_BAD_ARG.  These two checks come first and need no device.
 *   table       chunk i's pages are row_cnt[i] rows of eight int64 at rows + 8 * row_off[i] (host: at rows_ptrs[i]).  Read: word 0 —
 *               the low 32 bits the page type (0, 2 or 3), the high 32 bits V2's num_nulls (the pages query leaves them 0: a caller
 *               who has the value puts it there) —, word 3 uncompressed_page_size, word 5 num_values | num_rows << 32, word 6 the
 *               three encodings and bit 25, "write a crc for this page" (bit 24, is_compressed, is ignored: the writer decides it),
 *               word 7 the level lengths.  Words 1, 2 and 4 are ignored: a page's offset in the decoded chunk is the sum of word 3
 *               of the pages before it.
 *   result[i]   the written chunk's length or CJ_E_*, in this order: CJ_E_PARQUET_TABLE for row_cnt[i] > 0xFFFFFFF0;
 *               CJ_E_INPUT_TOO_LARGE for in_len[i] > 0x7E000000; CJ_E_PARQUET_TABLE at the first row in page order with a type
 *               outside {0, 2, 3}, a word 3 below 0 (or above 2^31 - 1), level lengths on a page that is not V2, or level lengths
 *               above word 3; CJ_E_PARQUET_TABLE when the sum of word 3 is not in_len[i]; the encoder's code of the first V1 or
 *               dictionary page in page order that has one; CJ_E_OUT_TOO_SMALL when the chunk would exceed out_cap[i].  All of it is
 *               decided before the chunk's first store: a chunk with a code writes NOTHING, and a capacity below the bound is allowed.
 *               A chunk of 0 pages and 0 bytes is an empty chunk, result 0.  One bad chunk never affects another.
 *   written     per page a PageHeader with its fields in ascending order and short form — 1 type, 2 uncompressed_page_size,
 *               3 compressed_page_size, 4 crc where asked for, then 5 DataPageHeader, 7 DictionaryPageHeader (without is_sorted) or
 *               8 DataPageHeaderV2 (is_compressed always written), no Statistics; 57 bytes at most (a V2 page: type 2; the sizes and
 *               the crc 6 each; the struct's header 1; num_values, num_nulls, num_rows 6 each; encoding 3; the level lengths 6 each;
 *               is_compressed 1; two stops) —, then a V2 page's levels copied from the input, then the values: 0 bytes for a values
 *               section of 0 bytes (the codec is not asked; is_compressed false); the bytes themselves for UNCOMPRESSED; else the
 *               codec's output (cj_batch_device for Snappy raw and raw LZ4 blocks, cj_deflate_compress_batch_* with CJ_DEFLATE_GZIP,
 *               cj_zstd_compress_batch_* without checksum) — but a V2 page whose output is not shorter than its values, or whose
 *               encoder reported an error, carries the raw values and is_compressed = false.  V1 and dictionary pages have no such
 *               flag and always carry the output.  The crc is gzip's CRC-32 of the payload as written, levels included.  The bytes
 *               depend on nothing but the input and the table.
 *   bound       cj_parquet_compress_bound(what, n_bytes, n_pages) = n_pages * (57 + K) + n_bytes + g(n_bytes), an upper bound over
 *               every way of cutting n_bytes into n_pages pages: a maximal header, the levels, and the codec's bound of the values,
 *               from the encoders' own bounds v + g(v) + K' with K' <= K — LZ4_RAW g = v / 255, K = 16; SNAPPY v / 6, 32; GZIP
 *               10 (v / 65536), 23; ZSTD 3 (v / 65536), 13; UNCOMPRESSED 0, 0.  0 for a bad `what`, n_bytes > 0x7E000000 or
 *               n_pages > 0xFFFFFFF0.  Pure arithmetic, no device.
 * NOT enqueue-only: a call takes one turn at the engine's container scratch and waits for the stream ONCE, for the chunks' plans
 * (page counts, pages the codec sees, slot bytes); the bound-sized page slots are engine scratch within a fixed budget, a large batch
 * runs in turns of whole chunks.  The _host call is cj_batch_host's one-shot staging, synchronous; a table of more rows than
 * 0x7E000000 / 64 that is not above 0xFFFFFFF0 is CJ_E_BAD_ARG there.  cj_parquet_batch_* with CJ_OP_COMPRESS stays CJ_E_BAD_ARG.
 * Not written: Statistics, footers, page indexes, bloom filters, Hadoop-framed LZ4, LZO, BROTLI; levels and values are not encoded. */
CJ_API int cj_parquet_compress_device(cj_engine* e, int what, uint32_t flags, size_t n_chunks,
                                      const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                      const int64_t* rows, const uint64_t* row_off, const uint64_t* row_cnt,
                                      uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                      int64_t* result, void* hip_stream);
CJ_API int cj_parquet_compress_host(cj_engine* e, int what, uint32_t flags, size_t n_chunks,
                                    const uint8_t* const* in_ptrs, const size_t* in_lens,
                                    const int64_t* const* rows_ptrs, const size_t* row_cnts,
                                    uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API size_t cj_parquet_compress_bound(int what, size_t n_bytes, size_t n_pages);

/* Zstandard frames — decode (RFC 8878; Parquet, ORC, Arrow IPC and Zarr v3 pages and chunks).  One chunk is what ONE call of
 * libzstd's ZSTD_decompress(dst, out_cap[i], src, in_len[i]) reads: one or more frames back to back, skippable frames skipped, an
 * empty input decoding to 0 bytes.  One wavefront decodes a chunk; result[i] and the bytes are libzstd's (1.4.x).
 * Addressing, the 16-byte-granule rule, stream rules, e == NULL, n_chunks == 0 and the null-pointer rules are cj_deflate_batch_*'s.
 *   fmt         a cj_zstd_format; anything else is CJ_E_BAD_ARG.       op   CJ_OP_DECOMPRESS, anything else is CJ_E_BAD_ARG.
 *   flags       0.  Any bit set is CJ_E_BAD_ARG.  These three checks come first and need no device.
 *   result[i]   the decoded length (>= 0) or CJ_E_*; one bad chunk never affects another; nothing is written at or behind
 *               out_base + out_off[i] + out_cap[i]; bytes between result[i] and out_cap[i] stay untouched (literals are staged in
 *               engine scratch, never in the caller's output).  in_len[i] > 0x7FFFFFF0 is CJ_E_CORRUPT, out_cap[i] > 0x7E000000 is
 *               CJ_E_PREFIX_TOO_BIG, in that chunk's own result[i].
 *   errors      libzstd's, in libzstd's order.  CJ_E_ZSTD_HEADER: a bad magic in the first frame (legacy v0.1 - v0.7 frames
 *               included), the reserved header bit, a window above 2^31.  CJ_E_ZSTD_DICT: a non-zero Dictionary_ID.
 *               CJ_E_ZSTD_SRC_SIZE: the input ends inside a frame, a bad magic behind a frame, 1 - 4 bytes left over, a compressed
 *               block of 128 KiB or more.  CJ_E_ZSTD_CORRUPT: a reserved block type, every rule of the literals and sequences
 *               sections (sizes, Huffman tree descriptions, streams that do not end as the one of libzstd's two Huffman decoders that libzstd picks wants, FSE descriptions, Repeat / Treeless
 *               without a table, an offset beyond the frame's output, literals that run out, a bitstream that does not end exactly),
 *               a Frame_Content_Size the blocks do not produce.  CJ_E_OUT_TOO_SMALL: a block, a sequence or the last literals do
 *               not fit.  CJ_E_ZSTD_CHECKSUM: the low 32 bits of XXH64 over the frame's output.
 *   sizes       the exact decoded length of a chunk that is valid; a total above 0x7E000000 is CJ_E_PREFIX_TOO_BIG.  A frame with a
 *               Frame_Content_Size contributes that number and only its block HEADERS are walked; in a frame without one the
 *               sequences sections are decoded and the literals skipped.  The query therefore does NOT report: CJ_E_ZSTD_CHECKSUM;
 *               in a frame with a content size, any CJ_E_ZSTD_CORRUPT cause but a reserved block type and the CJ_E_ZSTD_SRC_SIZE of a
 *               sequences header that its block cuts short; in a frame without one, what
 *               only decoding the literals finds (Huffman tree descriptions and streams, Treeless without a table).  A chunk the
 *               decoder refuses for one of these may get a size or a later error; every other verdict is the decoder's.
 * The _device calls only enqueue (a decode that has to GROW the engine's literal slots — one of 128 KiB + 32 per stream in flight,
 * within a fixed budget; a batch runs in slices of that many streams — waits for their previous user while it reallocates; the size
 * query uses no scratch).  The _host calls are cj_batch_host's one-shot staging, synchronous. */
typedef enum { CJ_ZSTD_FRAMES = 0 } cj_zstd_format;     /* room for magicless frames / raw blocks later */
CJ_API int cj_zstd_batch_device(cj_engine* e, cj_zstd_format fmt, cj_op op, uint32_t flags, size_t n_chunks,
                                const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                int64_t* result, void* hip_stream);
CJ_API int cj_zstd_batch_host(cj_engine* e, cj_zstd_format fmt, cj_op op, uint32_t flags, size_t n_chunks,
                              const uint8_t* const* in_ptrs, const size_t* in_lens,
                              uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API int cj_zstd_batch_sizes_device(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks,
                                      const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                      int64_t* result, void* hip_stream);
CJ_API int cj_zstd_batch_sizes_host(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks,
                                    const uint8_t* const* in_ptrs, const size_t* in_lens, int64_t* result);

/* Batches of inputs INTO Zstandard frames: one chunk in gives exactly one frame out — magic, a descriptor with
 * Frame_Content_Size always (Single_Segment up to 64 KiB, above that a Window_Descriptor of 64 KiB), no dictionary id, one block per
 * independent piece of at most 64 KiB (no match crosses a piece, distances up to 65 535): RLE when the piece is one repeated byte,
 * Compressed when its exact size is below the piece's, else Raw.  A Compressed block's literals are Raw, RLE or Huffman-coded (codes of
 * at most 11 bits, the tree as direct or FSE-compressed weights, one stream up to 1023 literals and four above), its sequences FSE-coded,
 * each table in RLE mode, FSE_Compressed or Predefined by an estimated cost; offsets are distance + 3 or the repeat code 1.  The bytes depend on nothing but the input and the
 * flag; an empty input gives a header and one empty last Raw block.  What cj_zstd_batch_* (libzstd's ZSTD_decompress) accepts is the
 * contract.  Addressing, the 16-byte-granule rule, stream rules, e == NULL, n_chunks == 0 and the null-pointer rules are
 * cj_deflate_compress_batch_*'s.
 *   fmt         CJ_ZSTD_FRAMES; anything else is CJ_E_BAD_ARG.      flags   0 or CJ_ZSTD_FLAG_CHECKSUM; any other bit is CJ_E_BAD_ARG.
 *   result[i]   the frame's length or CJ_E_*: in_len[i] > 0x7E000000 is CJ_E_INPUT_TOO_LARGE in that chunk's own result;
 *               CJ_E_OUT_TOO_SMALL when the frame does not fit out_cap[i] (checked per block from its exact size, before its first
 *               store: nothing is written at or behind out_cap[i]; what lies in the slot of such a chunk is unspecified).
 *   bound       cj_zstd_compress_bound(n, flags): the exact worst case of this layout, every piece a Raw block = the header (6 bytes
 *               for n <= 255, 7 up to 65 536, 8 up to 65 791, else 10) + 3 * max(1, ceil(n / 65536)) + n + 4 with the checksum
 *               <= n + 3 * (n / 65536 + 1) + 14; a capacity of that many bytes never gives CJ_E_OUT_TOO_SMALL.  0 for a bad flag or
 *               n > 0x7E000000.  Pure arithmetic, no device.
 * The _device call only enqueues (like every call, one that has to GROW the engine's scratch — the workgroups' record and literal
 * slots, within a fixed budget — waits for its previous user while it reallocates).  The _host call is cj_batch_host's one-shot
 * staging, synchronous.  cj_zstd_batch_* with CJ_OP_COMPRESS stays CJ_E_BAD_ARG. */
#define CJ_ZSTD_FLAG_CHECKSUM 1u     /* Content_Checksum: low 32 bits of XXH64 of the input behind the last block */
CJ_API int cj_zstd_compress_batch_device(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks,
                                         const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                         uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
                                         int64_t* result, void* hip_stream);
CJ_API int cj_zstd_compress_batch_host(cj_engine* e, cj_zstd_format fmt, uint32_t flags, size_t n_chunks,
                                       const uint8_t* const* in_ptrs, const size_t* in_lens,
                                       uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result);
CJ_API size_t cj_zstd_compress_bound(size_t n, uint32_t flags);

/* =====================================================================================
 * Blosc chunks (reference src/blosc2.rs:133-210 compress_chunk / decompress_chunk and their _into forms, :702-706
 * max_compressed_len): LZ4 streams behind a byte or bit transposition.  The transposition runs in its own kernels
 * (blosc_filters.hip), the streams of ALL chunks of a call go through the batch engine as one batch.
 *   READ     Blosc1-format chunks (c-blosc 1.x, format version 2, 16-byte header: what Zarr / numcodecs, PyTables and bcolz store,
 *            and what C-Blosc2 also reads) whose compressor format is LZ4 (codecs lz4 and lz4hc), filters none / shuffle / bitshuffle,
 *            typesize 1 .. 255, split and unsplit blocks, stored streams, memcpyed chunks (of any compressor format), the leftover block.
 *            With CJ_BLOSC_FLAG_READ_BLOSCLZ in a call's flags also chunks whose compressor format is BloscLZ (format 0, versionlz 1:
 *            c-blosc's default compressor, PyTables' complib="blosc"): the same container, each stream a byte-aligned LZ77 of the
 *            FastLZ family decoded by one wavefront (blosclz_decode.hip; the stream rules of c-blosc 1.21's blosclz_decompress).  One
 *            batch may mix LZ4 and BloscLZ chunks.  Without the flag (the default) such a chunk is refused as before.  BloscLZ is
 *            never written.
 *            With CJ_BLOSC_FLAG_READ_ZLIB / CJ_BLOSC_FLAG_READ_ZSTD also chunks whose compressor format is Zlib (format 3) / Zstd
 *            (format 4), versionlz 1 (c-blosc's cname "zlib" / "zstd": what most archival Zarr stores hold).  The container is the
 *            same; each stream that is not stored is one zlib-wrapped DEFLATE stream (CJ_DEFLATE_ZLIB, deflate.hip) / what one
 *            ZSTD_decompress call reads (zstd.hip), and is good iff it decodes to exactly its length: whatever CJ_E_DEFLATE_* /
 *            CJ_E_ZSTD_* code a stream produced, the chunk's result is CJ_E_CORRUPT.  One batch may mix all four formats.  Neither
 *            format is written.
 *   WRITTEN  the same format: blocks of 64 KiB x typesize split into typesize streams for typesize 2 .. 16 (else 64 KiB unsplit,
 *            flag 0x10), every stream at most 64 KiB; a stream that does not shrink is stored, a chunk that would not be smaller than
 *            nbytes + 16 (and every clevel 0 chunk) is memcpyed.  clevel 1 .. 9 select the one matcher of cj_batch_device.
 *   REFUSED  CJ_E_BLOSC_UNSUPPORTED: a format version other than 2 — above all C-Blosc2's extended 32-byte header (version > 2, with its
 *            filter pipeline: delta, truncated precision); nothing that writes such a chunk was at hand when this was built, so there is
 *            no decoder guessed from memory — and the compressor formats BloscLZ, Zlib, Zstd (each unless its flag above is set) and Snappy (always; on compress: any codec but
 *            CJ_BLOSC_LZ4 / CJ_BLOSC_LZ4HC, any filter but the three above).
 *            CJ_E_BLOSC_HEADER: a malformed container (short header, reserved flag, both shuffle bits, typesize 0, cbytes beyond the
 *            bytes given, blocksize 0 or above nbytes, a block start or stream word outside the chunk).
 *            CJ_E_CORRUPT: a stream that is not an LZ4 block (a BloscLZ stream, a zlib stream, a Zstandard frame) of exactly its length.  CJ_E_OUT_TOO_SMALL: nbytes above the capacity.
 *            A chunk refused for its header or its size writes nothing; one with a bad stream may have written inside its own slot.
 * ===================================================================================== */
typedef enum { CJ_BLOSC_NOFILTER = 0, CJ_BLOSC_SHUFFLE = 1, CJ_BLOSC_BITSHUFFLE = 2 } cj_blosc_filter;      /* the reference's Filter */
typedef enum { CJ_BLOSC_BLOSCLZ = 0, CJ_BLOSC_LZ4 = 1, CJ_BLOSC_LZ4HC = 2, CJ_BLOSC_ZLIB = 3, CJ_BLOSC_ZSTD = 4 } cj_blosc_codec;   /* its Codec */
typedef struct {
    uint32_t typesize;    /* 1 .. 255 */
    uint32_t filter;      /* cj_blosc_filter */
    int32_t clevel;       /* 0 .. 9; 0 = memcpyed chunk */
    uint32_t codec;       /* cj_blosc_codec: CJ_BLOSC_LZ4 or CJ_BLOSC_LZ4HC (the same streams) */
    uint32_t blocksize;   /* 0 = default; a value above the default block size is cut to it */
} cj_blosc_params;
typedef struct { uint32_t version, versionlz, flags, typesize, nbytes, blocksize, cbytes, nblocks; } cj_blosc_info;
/* flags of cj_blosc_batch_device / _host (decompress only) and cj_blosc_chunk_sizes_device / _host: any subset of the three below.
 * Bit 0 and bit 2 (value 4) are reserved; they and every higher bit are CJ_E_BAD_ARG, and so is any of these with CJ_OP_COMPRESS. */
#define CJ_BLOSC_FLAG_READ_BLOSCLZ 2u   /* also read chunks whose streams are BloscLZ */
#define CJ_BLOSC_FLAG_READ_ZLIB 8u      /* ... whose streams are zlib streams (compressor format 3) */
#define CJ_BLOSC_FLAG_READ_ZSTD 16u     /* ... whose streams are Zstandard frames (compressor format 4) */

/* src/blosc2.rs:702  upper bound of a chunk of n bytes: n + 32 (this library needs n + 16: the memcpyed chunk). No device. */
CJ_API size_t cj_blosc_chunk_max_compressed_len(size_t n);
/* the header of a chunk after its checks (0, CJ_E_BLOSC_HEADER or CJ_E_BLOSC_UNSUPPORTED; info is filled from the 16 bytes whenever
 * there are that many).  It takes no flags and reports the default reading: a BloscLZ, Zlib or Zstd chunk is CJ_E_BLOSC_UNSUPPORTED here
 * (info is still filled: flags >> 5 == 0 / 3 / 4 and versionlz == 1 name such a chunk).  No device. */
CJ_API int64_t cj_blosc_chunk_info(const uint8_t* in, size_t n, cj_blosc_info* info);
/* src/blosc2.rs:143,153  decompress_chunk / decompress_chunk_into: returns nbytes */
CJ_API int64_t cj_blosc_chunk_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t cap);
/* src/blosc2.rs:170,192  compress_chunk / compress_chunk_into: returns the chunk's size, CJ_E_COMPRESS_FAILED when cap is too small */
CJ_API int64_t cj_blosc_chunk_compress(const uint8_t* in, size_t n, uint8_t* out, size_t cap, const cj_blosc_params* params);
/* Batches of chunks, device-resident or on the host: addressing, alignment, stream rules and the one wait of cj_frame_batch_device /
 * _host (decompress reads back the chunks' stream counts, compress in_len).  result[i] = nbytes (decompress) / the chunk's size
 * (compress) or CJ_E_*; nothing is written outside out_off[i] .. + out_cap[i] (a chunk with a header or size error writes nothing at all).  params:
 * compress only (one set for the batch); flags: 0 or CJ_BLOSC_FLAG_READ_* (decompress only).  e == NULL: the default engine of device 0. */
CJ_API int cj_blosc_batch_device(cj_engine* e, cj_op op, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len,
                                 uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, size_t n_chunks,
                                 const cj_blosc_params* params, uint32_t flags, void* hip_stream);
CJ_API int cj_blosc_batch_host(cj_engine* e, cj_op op, uint32_t flags, size_t n_chunks, const uint8_t* const* in_ptrs, const size_t* in_lens,
                               uint8_t* const* out_ptrs, const size_t* out_caps, int64_t* result, const cj_blosc_params* params);
/* result[i] = nbytes of chunk i after the header checks of cj_blosc_chunk_info, or their error; flags as above (with
 * its CJ_BLOSC_FLAG_READ_* flag a BloscLZ, Zlib or Zstd chunk reports its nbytes).  Enqueue-only like cj_batch_sizes_device. */
CJ_API int cj_blosc_chunk_sizes_device(cj_engine* e, uint32_t flags, size_t n_chunks, const uint8_t* in_base, const uint64_t* in_off,
                                       const uint64_t* in_len, int64_t* result, void* hip_stream);
CJ_API int cj_blosc_chunk_sizes_host(cj_engine* e, uint32_t flags, size_t n_chunks, const uint8_t* const* in_ptrs, const size_t* in_lens,
                                     int64_t* result);

/* Thin device-memory helpers so C / ctypes callers need no HIP binding of their own.  Each returns when its bytes are in place
 * (cj_memset_dev and cj_memcpy_d2d wait for the null stream: an engine's stream is non-blocking and would not). */
CJ_API void* cj_device_alloc(cj_engine* e, size_t bytes);
CJ_API void  cj_device_free(cj_engine* e, void* p);
CJ_API int   cj_memcpy_h2d(cj_engine* e, void* dst_dev, const void* src_host, size_t bytes);
CJ_API int   cj_memcpy_d2h(cj_engine* e, void* dst_host, const void* src_dev, size_t bytes);
CJ_API int   cj_memcpy_d2d(cj_engine* e, void* dst_dev, const void* src_dev, size_t bytes);
CJ_API int   cj_memset_dev(cj_engine* e, void* dst_dev, int value, size_t bytes);

/* The test / benchmark utilities and debug counters the library also exports (cj_bench_*, cj_debug_*) are declared in
 * cramjam_hip_debug.h: they are NOT part of the drop-in ABI. */

#ifdef __cplusplus
}
#endif
#endif
