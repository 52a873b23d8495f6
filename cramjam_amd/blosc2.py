"""Blosc chunks on the MI355X: the chunk API of the reference's `blosc2` module (src/blosc2.rs:133-210, :592-680, :702-706) —
`compress_chunk`, `compress_chunk_into`, `decompress_chunk`, `decompress_chunk_into`, `max_compressed_len` and the enums `Filter`,
`CLevel`, `Codec` — as the single-chunk case of the chunk batches (cramjam_amd.batch.blosc_*; C-ABI cj_blosc_chunk_*).

What is read and written: Blosc1-format chunks (16-byte header, format version 2) whose streams are LZ4, behind no filter, the
byte shuffle or the bitshuffle.  With `blosclz=True` the decompress calls also read chunks whose streams are BloscLZ (c-blosc's default
compressor, what the reference's `compress_chunk` writes by default); it is off by default, and BloscLZ is never written.
`zlib=True` and `zstd=True` do the same for chunks whose streams are zlib streams and Zstandard frames (c-blosc's cname "zlib" and
"zstd", the reference's `Codec.ZLIB` / `Codec.ZSTD` on decompress: what `Blosc(cname="zstd")` of Zarr / numcodecs stores); neither is
written.  Refused with an error (never a wrong result): the other compressor formats (BloscLZ, Zlib, Zstd without their keyword,
Snappy always; on compress `Codec.BloscLz / ZLIB / ZSTD`), `Filter.Delta / TruncPrec`, and C-Blosc2's extended 32-byte header.  Not here:
`SChunk`, the `compress` / `decompress` frame container, `Compressor` / `Decompressor`, `set_nthreads`.
Deviations: `codec=None` means LZ4 (the reference's default is BloscLZ; every Blosc reader decodes either); `clevel` 1-9 select the
one matcher of the engine, `clevel=0` stores; `typesize=None` is the itemsize of the buffer handed in (1 for `bytes`) as the
reference's `Chunk.compress` does — what its plain `compress_chunk` does with None lies in a crate that was not at hand."""
import enum as _enum

from . import _native as _N

__all__ = ["compress_chunk", "compress_chunk_into", "decompress_chunk", "decompress_chunk_into", "max_compressed_len", "Filter", "CLevel", "Codec"]


class Filter(_enum.IntEnum):
    NoFilter = 0
    Shuffle = 1
    BitShuffle = 2
    Delta = 3
    TruncPrec = 4
    LastFilter = 5
    LastRegisteredFilter = 6


class CLevel(_enum.IntEnum):
    Zero = 0
    One = 1
    Two = 2
    Three = 3
    Four = 4
    Five = 5
    Six = 6
    Seven = 7
    Eight = 8
    Nine = 9


class Codec(_enum.IntEnum):
    BloscLz = 0
    LZ4 = 1
    LZ4HC = 2
    ZLIB = 3
    ZSTD = 4
    LastCodec = 5
    LastRegisteredCodec = 6


def _errors():
    from . import _cramjam
    return _cramjam.CompressionError, _cramjam.DecompressionError


def _params(typesize, clevel, filter, codec, blocksize=0):
    typesize = 1 if typesize is None else int(typesize)
    if not 1 <= typesize <= 255:
        raise ValueError("blosc2: typesize must be 1 .. 255, got %d" % typesize)
    clevel = 5 if clevel is None else int(clevel)
    if not 0 <= clevel <= 9:
        raise ValueError("blosc2: clevel must be 0 .. 9, got %d" % clevel)
    return _N.BloscParams(typesize, int(Filter.Shuffle if filter is None else filter), clevel, int(Codec.LZ4 if codec is None else codec), int(blocksize))


def _view(data):
    """(contiguous byte view, itemsize of what was handed in)"""
    mv = memoryview(data)
    return (mv if mv.ndim == 1 and mv.format == "B" and mv.contiguous else mv.cast("B")), mv.itemsize


def _raise(exc, rc):
    raise exc("blosc2: %s" % _N.strerror(rc))


def _one(op, data, cap, out, params, exc, blosclz=False, zlib=False, zstd=False):
    from .batch import _engine
    flags = _N.BLOSC.read_flags(blosclz, zlib, zstd)
    try:
        eng = _engine(0)
        if out is None:
            res, outs = eng.batch_host(0, op, flags, [data], [cap], _N.BLOSC, params)
        else:
            res, outs = eng.batch_host_into(0, op, flags, [data], [cap], out, None, _N.BLOSC, params), None
    except _N.EngineError as ex:
        raise RuntimeError(str(ex)) from None
    if res[0] < 0:
        _raise(exc, res[0])
    return res[0], outs


def max_compressed_len(len_bytes):
    """upper bound of the chunk of `len_bytes` bytes: len_bytes + 32"""
    return _N.lib().cj_blosc_chunk_max_compressed_len(int(len_bytes))


def compress_chunk(data, typesize=None, clevel=None, filter=None, codec=None):
    """Blosc compression, chunk format -> cramjam.Buffer"""
    from . import _cramjam
    mv, item = _view(data)
    p = _params(item if typesize is None else typesize, clevel, filter, codec)
    _, outs = _one(_N.OP_COMPRESS, mv, mv.nbytes + 32, None, bytes(p), _errors()[0])
    return _cramjam.Buffer(outs[0])


def compress_chunk_into(input, output, typesize=None, clevel=None, filter=None, codec=None):
    """Compress a chunk into `output`; returns the chunk's size"""
    mv, item = _view(input)
    out = memoryview(output).cast("B")
    p = _params(item if typesize is None else typesize, clevel, filter, codec)
    return _one(_N.OP_COMPRESS, mv, out.nbytes, out, bytes(p), _errors()[0])[0]


def _info_nbytes(addr, n, blosclz=False, zlib=False, zstd=False):
    """(cj_blosc_chunk_info's code, nbytes) of a chunk on the host.  cj_blosc_chunk_info reports the default reading; with `blosclz`,
    `zlib` or `zstd` the one refusal that keyword lifts — compressor format 0, 3 or 4 with versionlz 1, the last check before the block
    table's — is taken back here.  The decode call checks the whole chunk again with the flags."""
    import ctypes as C
    info = _N.BloscInfo()
    rc = _N.lib().cj_blosc_chunk_info(addr, n, C.byref(info))
    opted = {0: blosclz, 3: zlib, 4: zstd}.get(info.flags >> 5, False)
    if rc == _N.E_BLOSC_UNSUPPORTED and opted and info.version == 2 and info.versionlz == 1 and not info.flags & 2:
        rc = 0
    return rc, info.nbytes


def _nbytes(mv, exc, blosclz=False, zlib=False, zstd=False):
    import numpy as np
    a = np.frombuffer(mv, dtype=np.uint8)
    rc, nbytes = _info_nbytes(a.ctypes.data if a.size else None, a.size, blosclz, zlib, zstd)
    if rc != 0:
        _raise(exc, rc)
    return nbytes


def decompress_chunk(data, output_len=None, blosclz=False, zlib=False, zstd=False):
    """Blosc chunk decompression -> cramjam.Buffer (output_len is accepted and ignored, as in the reference: the chunk names its size).
    blosclz=True / zlib=True / zstd=True: a chunk whose streams are BloscLZ / zlib streams / Zstandard frames is decoded too (the
    default refuses each as unsupported)"""
    from . import _cramjam
    mv, _ = _view(data)
    exc = _errors()[1]
    _, outs = _one(_N.OP_DECOMPRESS, mv, _nbytes(mv, exc, blosclz, zlib, zstd), None, b"", exc, blosclz, zlib, zstd)
    return _cramjam.Buffer(outs[0])


def decompress_chunk_into(input, output, blosclz=False, zlib=False, zstd=False):
    """Decompress a chunk into `output`; returns nbytes.  blosclz, zlib, zstd: as in decompress_chunk"""
    mv, _ = _view(input)
    out = memoryview(output).cast("B")
    return _one(_N.OP_DECOMPRESS, mv, out.nbytes, out, b"", _errors()[1], blosclz, zlib, zstd)[0]
