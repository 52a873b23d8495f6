"""ctypes binding of libcramjam_hip.so (include/cramjam_hip.h).  The library is the product; if it is
missing or no HIP device is usable every compute call fails loudly — there is no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CJ_HIP_LIB") or os.path.join(_HERE, "libcramjam_hip.so")   # CJ_HIP_LIB: a tuning variant (tools/build_variant.sh)

CODEC_LZ4_BLOCK, CODEC_SNAPPY_RAW = 0, 1
FORMAT_LZ4_FRAME, FORMAT_SNAPPY_FRAMED = 0, 1      # cj_frame_batch_*
OP_DECOMPRESS, OP_COMPRESS = 0, 1
DEFLATE_RAW, DEFLATE_ZLIB, DEFLATE_GZIP = 0, 1, 2  # cj_deflate_wrap (cj_deflate_batch_*)
FLAG_LZ4_SIZE_PREFIX = 1
FLAG_FORCE_WAVE_PER_CHUNK = 0x100
FLAG_FORCE_LANE_PER_CHUNK = 0x200
FLAG_FORCE_LDS_PER_CHUNK = 0x400
FLAG_FORCE_FUSED_PARSE = 0x10     # the workgroup decoder's parse stage inside the decoder kernel / as its own kernel, at any batch size
FLAG_FORCE_PARSE_KERNEL = 0x20
FLAG_CHUNKS_LE_32K = 0x40          # decompress: a promise that no chunk is larger (windows of that size: more workgroups per CU); host batches set them themselves
FLAG_CHUNKS_LE_16K = 0x80
FLAG_BIG_CHUNKS = 0x800            # decompress: reserve record areas for chunks of 64 KiB .. 256 KiB (cramjam_hip.h)
E_NO_DEVICE = -100
E_BLOSC_HEADER, E_BLOSC_UNSUPPORTED = -30, -31
E_DEFLATE_CORRUPT, E_DEFLATE_HEADER, E_DEFLATE_CHECKSUM, E_DEFLATE_EOF, E_DEFLATE_TRAILING = -40, -41, -42, -43, -44
E_ZSTD_HEADER, E_ZSTD_CORRUPT, E_ZSTD_CHECKSUM, E_ZSTD_SRC_SIZE, E_ZSTD_DICT = -50, -51, -52, -53, -54
E_ORC_HEADER, E_ORC_BLOCK = -60, -61
E_PARQUET_HEADER, E_PARQUET_SIZE, E_PARQUET_CRC, E_PARQUET_TABLE = -70, -71, -72, -73
ORC_ZLIB, ORC_SNAPPY, ORC_LZ4, ORC_ZSTD = 1, 2, 4, 5      # ORC's CompressionKind (cj_orc_batch_*)
PARQUET_UNCOMPRESSED, PARQUET_SNAPPY, PARQUET_GZIP, PARQUET_ZSTD, PARQUET_LZ4_RAW = 0, 1, 2, 6, 7      # Parquet's CompressionCodec (cj_parquet_batch_*)
PARQUET_FLAG_VERIFY_CRC = 1        # cj_parquet_batch_*: check the CRC-32 of every page that carries one
ZSTD_FRAMES = 0                    # cj_zstd_format (cj_zstd_batch_*)
ZSTD_FLAG_CHECKSUM = 1             # cj_zstd_compress_batch_*: a Content_Checksum behind the last block
BLOSC_FLAG_READ_BLOSCLZ = 2        # cj_blosc_batch_* (decompress) / cj_blosc_chunk_sizes_*: also read chunks whose streams are BloscLZ
BLOSC_FLAG_READ_ZLIB = 8           # ... zlib streams (compressor format 3)
BLOSC_FLAG_READ_ZSTD = 16          # ... Zstandard frames (compressor format 4)


class BloscParams(C.Structure):
    """cj_blosc_params"""
    _fields_ = [("typesize", C.c_uint32), ("filter", C.c_uint32), ("clevel", C.c_int32), ("codec", C.c_uint32), ("blocksize", C.c_uint32)]


class BloscInfo(C.Structure):
    """cj_blosc_info"""
    _fields_ = [(n, C.c_uint32) for n in ("version", "versionlz", "flags", "typesize", "nbytes", "blocksize", "cbytes", "nblocks")]


_vp, _sz, _i64, _u32, _int = C.c_void_p, C.c_size_t, C.c_int64, C.c_uint32, C.c_int

# every symbol include/cramjam_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "cj_strerror": (C.c_char_p, [_i64]),
    "cj_last_hip_error": (C.c_char_p, []),
    "cj_abi_version": (_int, []),
    "cj_device_count": (_int, []),
    "cj_lz4_block_compress_bound": (_sz, [_sz, _int]),
    "cj_lz4_block_compress": (_i64, [_vp, _sz, _vp, _sz, _int, _int, _int]),
    "cj_lz4_block_decompress": (_i64, [_vp, _sz, _vp, _sz, _int]),
    "cj_lz4_block_prefixed_len": (_i64, [_vp, _sz]),
    "cj_snappy_raw_max_compress_len": (_sz, [_sz]),
    "cj_snappy_raw_decompress_len": (_i64, [_vp, _sz]),
    "cj_snappy_raw_compress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_snappy_raw_decompress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_snappy_frame_max_compress_len": (_sz, [_sz]),
    "cj_snappy_frame_compress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_snappy_frame_decompress_len": (_i64, [_vp, _sz]),
    "cj_snappy_frame_decompress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_lz4_frame_compress_bound": (_sz, [_sz]),
    "cj_lz4_frame_compress": (_i64, [_vp, _sz, _vp, _sz, C.c_int]),
    "cj_lz4_frame_compress_blocks": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_lz4_frame_compress_linked": (_i64, [_vp, _sz, _vp, _sz, C.c_int]),
    "cj_lz4_frame_compress_blocks_linked": (_i64, [_vp, _sz, _vp, _sz, _vp, _sz]),
    "cj_lz4_frame_decompress_bound": (_i64, [_vp, _sz]),
    "cj_lz4_frame_decompress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_engine_create": (_int, [_int, C.POINTER(_vp)]),
    "cj_engine_destroy": (None, [_vp]),
    "cj_engine_device": (_int, [_vp]),
    "cj_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_engine_sync": (_int, [_vp]),
    "cj_stream_sync": (_int, [_vp, _vp]),
    "cj_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_frame_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_frame_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_batch_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_batch_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_frame_batch_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_frame_batch_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_dict_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cj_dict_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "cj_dict_batch_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cj_dict_batch_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _sz]),
    "cj_deflate_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_deflate_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_deflate_batch_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_deflate_batch_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_zstd_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_zstd_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_zstd_batch_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_zstd_batch_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_deflate_compress_batch_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_deflate_compress_batch_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_deflate_compress_bound": (_sz, [_sz, _int]),
    "cj_bgzf_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_bgzf_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_bgzf_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_bgzf_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_bgzf_compress_bound": (_sz, [_sz]),
    "cj_orc_batch_device": (_int, [_vp, _int, _int, _u32, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_orc_batch_host": (_int, [_vp, _int, _int, _u32, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_orc_sizes_device": (_int, [_vp, _int, _u32, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_orc_sizes_host": (_int, [_vp, _int, _u32, _u32, _sz, _vp, _vp, _vp]),
    "cj_orc_compress_bound": (_sz, [_sz, _u32]),
    "cj_parquet_batch_device": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_batch_host": (_int, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_sizes_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_sizes_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp]),
    "cj_parquet_pages_device": (_int, [_vp, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_pages_host": (_int, [_vp, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_compress_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_compress_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_parquet_compress_bound": (_sz, [_int, _sz, _sz]),
    "cj_zstd_compress_batch_device": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_zstd_compress_batch_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_zstd_compress_bound": (_sz, [_sz, _u32]),
    "cj_batch_device_timed": (C.c_double, [_vp, _int, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int]),
    "cj_blosc_chunk_max_compressed_len": (_sz, [_sz]),
    "cj_blosc_chunk_info": (_i64, [_vp, _sz, _vp]),
    "cj_blosc_chunk_decompress": (_i64, [_vp, _sz, _vp, _sz]),
    "cj_blosc_chunk_compress": (_i64, [_vp, _sz, _vp, _sz, _vp]),
    "cj_blosc_batch_device": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _u32, _vp]),
    "cj_blosc_batch_host": (_int, [_vp, _int, _u32, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cj_blosc_chunk_sizes_device": (_int, [_vp, _u32, _sz, _vp, _vp, _vp, _vp, _vp]),
    "cj_blosc_chunk_sizes_host": (_int, [_vp, _u32, _sz, _vp, _vp, _vp]),
    "cj_device_alloc": (_vp, [_vp, _sz]),
    "cj_device_free": (None, [_vp, _vp]),
    "cj_memcpy_h2d": (_int, [_vp, _vp, _vp, _sz]),
    "cj_memcpy_d2h": (_int, [_vp, _vp, _vp, _sz]),
    "cj_memcpy_d2d": (_int, [_vp, _vp, _vp, _sz]),
    "cj_memset_dev": (_int, [_vp, _vp, _int, _sz]),
}
# benchmark/test utilities exported next to the engine (include/cramjam_hip_debug.h); not part of the drop-in ABI
BENCH_SYMBOLS = {
    "cj_bench_synth_v1": (_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _vp]),
    "cj_debug_lds_phase_cycles": (_int, [_vp, _int]),
    "cj_debug_linked_lds_frames": (C.c_ulonglong, []),
    "cj_debug_forwarded_chunks": (C.c_longlong, [_int]),
    "cj_debug_fused_parse_paths": (_int, [_vp, _int]),
    "cj_debug_big_parse": (C.c_int64, [_int, _u32, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "cj_bench_compare": (_int, [_vp, _vp, _vp, C.c_uint64, _u32, C.c_uint64, _u32, _vp, _vp]),
    "cj_debug_big_scratch_bytes": (C.c_uint64, [_vp]),
    "cj_debug_scratch_count": (_int, []),
    "cj_debug_scratch_name": (C.c_char_p, [_int]),
    "cj_debug_scratch_carries_state": (_int, [_int]),
    "cj_debug_scratch_fill": (_int, [_vp, _u32, _vp]),
    "cj_debug_scratch_peek": (_int, [_vp, _int, C.c_uint64, _vp, _sz]),
    "cj_debug_xxh32_device":(_int, [_vp, _vp, _vp, _vp, _vp, _sz]),
    "cj_debug_blosc_filter": (_int, [_vp, _int, _u32, _u32, _vp, _vp, C.c_uint64, C.c_uint64, _sz, _vp]),
    "cj_debug_dict_stage_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_deflate_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_bgzf_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_orc_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_parquet_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_zstd_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_zstd_enc_slot_budget": (C.c_uint64, [C.c_uint64]),
    "cj_debug_grid_chunks": (C.c_uint64, [C.c_uint64]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "cramjam_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(BENCH_SYMBOLS.items()):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def strerror(code):
    return lib().cj_strerror(code).decode()


class EngineError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise EngineError("%s (%s)" % (strerror(rc), lib().cj_last_hip_error().decode()))


def _with_hip_error(msg):
    """the host module's message and the HIP error text behind it — from THIS library's thread-local slot: the module's calls go through
    this library's entry points (_batch_host_addr), so the text lies here and not in the library the module links"""
    return "%s (%s)" % (msg, lib().cj_last_hip_error().decode())


def _batch_host_addr(name="cj_batch_host"):
    """address of a host-batch entry (a Kind's .host) in the library the engines of this process come from (CJ_HIP_LIB may name a tuning
    variant; the CPython module links the product library)"""
    return C.cast(getattr(lib(), name), C.c_void_p).value


class Kind:
    """One kind of batch: its four C symbols, and how `what` (a CODEC_* / FORMAT_*; Blosc chunks have none), `params` (a BloscParams
    or None) and `extra` enter their argument lists.  i = (in_base, in_off, in_len) / (in_ptrs, in_lens); o = (out_base, out_off, out_cap)."""

    def __init__(self, host, device, sizes_host, sizes_device, blosc=False, dictionary=False, one_op=False, extra=False):
        self.host, self.device, self.sizes_host, self.sizes_device, self.blosc = host, device, sizes_host, sizes_device, blosc
        self.one_op = one_op                        # the calls have one direction: their argument lists carry no `op`
        self.extra = extra                          # the calls carry one uint32_t of their own directly behind `flags` (ORC: block_size)
        self.dictionary = dictionary                # the calls take (dict, dict_len) / (dict_len,) behind result: `params` = that tuple

    def read_flags(self, blosclz=False, zlib=False, zstd=False):
        """the flags word of a reading call of this kind: `blosclz`, `zlib`, `zstd` (Blosc chunks only) ask for chunks whose streams are
        BloscLZ, zlib streams or Zstandard frames to be read too"""
        if (blosclz or zlib or zstd) and not self.blosc:
            raise ValueError("blosclz, zlib and zstd apply to Blosc chunks only")
        return (BLOSC_FLAG_READ_BLOSCLZ if blosclz else 0) | (BLOSC_FLAG_READ_ZLIB if zlib else 0) | (BLOSC_FLAG_READ_ZSTD if zstd else 0)

    def _flags(self, flags, extra):
        return (flags, extra) if self.extra else (flags,)

    def device_args(self, h, what, op, flags, n, i, o, result, params, stream, extra=None):
        if self.blosc:                              # (cj_blosc_batch_device has an argument order of its own)
            return (h, op) + i + o + (result, n, C.byref(params) if params is not None else None, flags, stream)
        head = ((h, what) if self.one_op else (h, what, op)) + self._flags(flags, extra) + (n,)
        return head + i + o + (result,) + (tuple(params) if self.dictionary else ()) + (stream,)

    def sizes_args(self, h, what, flags, n, body, tail=(), dict_len=0, extra=None):
        """body = i + (result,); tail = (stream,) for the device form; dict_len (dictionary batches only) goes between them"""
        return ((h,) if self.blosc else (h, what)) + self._flags(flags, extra) + (n,) + body + ((dict_len,) if self.dictionary else ()) + tail


BLOCKS = Kind("cj_batch_host", "cj_batch_device", "cj_batch_sizes_host", "cj_batch_sizes_device")
FRAMES = Kind("cj_frame_batch_host", "cj_frame_batch_device", "cj_frame_batch_sizes_host", "cj_frame_batch_sizes_device")
DICT = Kind("cj_dict_batch_host", "cj_dict_batch_device", "cj_dict_batch_sizes_host", "cj_dict_batch_sizes_device", dictionary=True)
DEFLATE = Kind("cj_deflate_batch_host", "cj_deflate_batch_device", "cj_deflate_batch_sizes_host", "cj_deflate_batch_sizes_device")   # what = a DEFLATE_*
DEFLATE_COMPRESS = Kind("cj_deflate_compress_batch_host", "cj_deflate_compress_batch_device", None, None, one_op=True)      # what = a DEFLATE_*; no size query
ZSTD = Kind("cj_zstd_batch_host", "cj_zstd_batch_device", "cj_zstd_batch_sizes_host", "cj_zstd_batch_sizes_device")   # what = ZSTD_FRAMES
ZSTD_COMPRESS = Kind("cj_zstd_compress_batch_host", "cj_zstd_compress_batch_device", None, None, one_op=True)      # what = ZSTD_FRAMES; no size query
BGZF = Kind("cj_bgzf_batch_host", "cj_bgzf_batch_device", "cj_bgzf_sizes_host", "cj_bgzf_sizes_device")   # what = 0; both directions
ORC = Kind("cj_orc_batch_host", "cj_orc_batch_device", "cj_orc_sizes_host", "cj_orc_sizes_device", extra=True)   # what = an ORC_*; extra = block_size
PARQUET = Kind("cj_parquet_batch_host", "cj_parquet_batch_device", "cj_parquet_sizes_host", "cj_parquet_sizes_device")   # what = a PARQUET_*; decode only; flags: PARQUET_FLAG_VERIFY_CRC.  The pages query (cj_parquet_pages_*) has a call shape of its own: batch.parquet_pages
BLOSC = Kind("cj_blosc_batch_host", "cj_blosc_batch_device", "cj_blosc_chunk_sizes_host", "cj_blosc_chunk_sizes_device", blosc=True)
_HOST_KINDS = {k.host: k for k in (BLOCKS, FRAMES, DICT, DEFLATE, DEFLATE_COMPRESS, ZSTD, ZSTD_COMPRESS, BGZF, ORC, PARQUET, BLOSC)}


class Engine:
    """One engine per GPU (cj_engine).  Thin: device memory + batch submission."""

    def __init__(self, device=0):
        h = _vp()
        check(lib().cj_engine_create(device, C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().cj_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, nbytes):
        p = lib().cj_device_alloc(self.h, nbytes)
        if not p:
            raise EngineError("device alloc of %d bytes failed: %s" % (nbytes, lib().cj_last_hip_error().decode()))
        return p

    def free(self, p):
        lib().cj_device_free(self.h, p)

    def h2d(self, dptr, data):
        import numpy as np
        a = np.ascontiguousarray(data)
        check(lib().cj_memcpy_h2d(self.h, dptr, a.ctypes.data, a.nbytes))

    def d2h(self, dptr, nbytes, dtype="uint8"):
        import numpy as np
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        check(lib().cj_memcpy_d2h(self.h, out.ctypes.data, dptr, out.nbytes))
        return out

    def memset(self, dptr, value, nbytes):
        check(lib().cj_memset_dev(self.h, dptr, value, nbytes))

    def sync(self):
        check(lib().cj_engine_sync(self.h))

    def batch_device(self, codec, op, flags, n, in_base, in_off, in_len, out_base, out_off, out_cap, result, stream=None):
        check(lib().cj_batch_device(self.h, codec, op, flags, n, in_base, in_off, in_len, out_base, out_off,
                                    out_cap, result, stream))

    def batch_device_timed(self, codec, op, flags, n, in_base, in_off, in_len, out_base, out_off, out_cap, result, reps):
        ms = lib().cj_batch_device_timed(self.h, codec, op, flags, n, in_base, in_off, in_len, out_base, out_off,
                                         out_cap, result, reps)
        if ms < 0:
            raise EngineError("timed batch failed: %s" % lib().cj_last_hip_error().decode())
        return ms

    def frame_batch_device(self, fmt, op, flags, n, in_base, in_off, in_len, out_base, out_off, out_cap, result, stream=None):
        check(lib().cj_frame_batch_device(self.h, fmt, op, flags, n, in_base, in_off, in_len, out_base, out_off,
                                          out_cap, result, stream))

    def _host(self, entry, codec, op, flags, args, fn, params, dictionary, extra=None):
        """entry: batch_host or batch_host_into of the CPython host layer (the engine scatters straight into the bytes objects / the buffer).
        fn: a Kind, or the name of its host entry — the call's signature is the Kind's: BLOSC takes params, the bytes of a cj_blosc_params
        (b"" = decompress; codec is not used), DICT a dictionary, bytes-like (borrowed), DEFLATE_COMPRESS and ZSTD_COMPRESS have no op, ORC takes
        extra, its block_size, an int.  None: DICT with a dictionary, BLOSC with params, else BLOCKS.  An argument the Kind does not take: ValueError."""
        from . import _cramjam
        if fn is None:
            fn = DICT if dictionary is not None else BLOSC if params is not None else BLOCKS
        kind = fn if isinstance(fn, Kind) else _HOST_KINDS[fn]
        if (params is not None and not kind.blosc) or (dictionary is not None and not kind.dictionary):
            raise ValueError("cramjam_amd: %s takes no %s" % (kind.host, "params" if params is not None and not kind.blosc else "dictionary"))
        if (extra is not None) != kind.extra:
            raise ValueError("cramjam_amd: %s takes %s extra word" % (kind.host, "an" if kind.extra else "no"))
        try:
            return getattr(_cramjam, entry)(self.h.value or 0, 0 if kind.blosc else int(codec), int(op), int(flags), *args, _batch_host_addr(kind.host),
                                            params, dictionary, kind.one_op, extra)
        except RuntimeError as ex:                  # (a CJ_E_* return code of the call itself, not of a chunk)
            raise EngineError(_with_hip_error(str(ex))) from None

    def batch_host(self, codec, op, flags, inputs, out_caps, fn=None, params=None, dictionary=None, extra=None):
        """inputs: list of bytes-like (anything with the buffer protocol: borrowed, not copied); out_caps: list of capacities.
        Returns (results, outputs): results[i] = bytes produced or a negative CJ_E_* code, outputs[i] = bytes.
        fn: the Kind of the batch or the name of its host entry, "cj_frame_batch_host" for batches of framed streams (codec is then a FORMAT_*).
        extra: the uint32_t a Kind with `extra` carries behind flags (N.ORC: the block size)."""
        return self._host("batch_host", codec, op, flags, (inputs, out_caps), fn, params, dictionary, extra)

    def batch_host_into(self, codec, op, flags, inputs, out_caps, out, offsets=None, fn=None, params=None, dictionary=None, extra=None):
        """the same batch into ONE writable buffer (bytearray, numpy array, ...): chunk i at out[offsets[i] : offsets[i] + out_caps[i]],
        back to back when offsets is None.  Returns results."""
        return self._host("batch_host_into", codec, op, flags, (inputs, out_caps, out, offsets), fn, params, dictionary, extra)
