"""Zstandard frames on the MI355X: the one-shot calls of the reference's `zstd` module (src/cramjam/zstd.pyi: `compress`,
`decompress`, `compress_into`, `decompress_into`) as the single-buffer case of the frame batches (cramjam_amd.batch.zstd_compress_many /
zstd_decompress_many; C-ABI cj_zstd_compress_batch_* / cj_zstd_batch_*).

What is written: one frame per call with Frame_Content_Size, independent pieces of 64 KiB, no content checksum (the batch call has the
flag).  There is ONE compression level: `level` is accepted and validated as an int or None like the reference's, and does not
change the bytes.  What is read: what libzstd's ZSTD_decompress reads — one or more frames, skippable frames skipped, checksums
verified; frames that name a dictionary are refused.  Not here: the streaming `Compressor` / `Decompressor` of the reference's module."""
from . import _native as _N

__all__ = ["compress", "decompress", "compress_into", "decompress_into"]

_NAMES = {-1: "CJ_E_INPUT_TOO_LARGE", -6: "CJ_E_OUT_TOO_SMALL", -50: "CJ_E_ZSTD_HEADER", -51: "CJ_E_ZSTD_CORRUPT", -52: "CJ_E_ZSTD_CHECKSUM",
          -53: "CJ_E_ZSTD_SRC_SIZE", -54: "CJ_E_ZSTD_DICT"}


def _errors():
    from . import _cramjam
    return _cramjam.CompressionError, _cramjam.DecompressionError


def _view(data):
    """a contiguous byte view of bytes / bytearray / Buffer / numpy arrays ...; a File is read from its cursor to its end"""
    from . import _cramjam
    if isinstance(data, _cramjam.File):
        data = data.read()
    mv = memoryview(data)
    return mv if mv.ndim == 1 and mv.format == "B" and mv.contiguous else mv.cast("B")


def _level(level):
    if level is not None and (isinstance(level, bool) or not isinstance(level, int)):
        raise TypeError("zstd: level must be an int or None, not %s" % type(level).__name__)


def _raise(exc, rc):
    raise exc("zstd: %s: %s" % (_NAMES.get(rc, "CJ_E_%d" % -rc), _N.strerror(rc)))


def _one(kind, op, data, cap, out, exc):
    from .batch import _engine
    try:
        eng = _engine(0)
        if out is None:
            res, outs = eng.batch_host(_N.ZSTD_FRAMES, op, 0, [data], [cap], kind)
        else:
            res, outs = eng.batch_host_into(_N.ZSTD_FRAMES, op, 0, [data], [cap], out, None, kind), None
    except _N.EngineError as ex:
        raise RuntimeError(str(ex)) from None
    if res[0] < 0:
        _raise(exc, res[0])
    return res[0], outs


def _bound(n, exc):
    b = _N.lib().cj_zstd_compress_bound(n, 0)
    if b == 0:
        _raise(exc, -1)
    return b


def _size(mv, exc):
    from .batch import zstd_sizes
    try:
        n = zstd_sizes([mv])[0]
    except _N.EngineError as ex:
        raise RuntimeError(str(ex)) from None
    if n < 0:
        _raise(exc, n)
    return n


def _into(output, produce):
    """produce(writable byte view or None) -> (length, bytes or None); a File takes the bytes through its write()"""
    from . import _cramjam
    if isinstance(output, _cramjam.File):
        n, outs = produce(None)
        output.write(outs[0][:n])
        return n
    return produce(memoryview(output).cast("B"))[0]


def compress(data, level=None, output_len=None):
    """zstd compression -> cramjam.Buffer.  `level` is accepted (an int or None) and does not change the bytes: the engine has one
    level.  output_len: the capacity to compress into (None: the bound, which always suffices)"""
    from . import _cramjam
    _level(level)
    mv, exc = _view(data), _errors()[0]
    n, outs = _one(_N.ZSTD_COMPRESS, _N.OP_COMPRESS, mv, _bound(mv.nbytes, exc) if output_len is None else int(output_len), None, exc)
    return _cramjam.Buffer(outs[0][:n])


def decompress(data, output_len=None):
    """zstd decompression -> cramjam.Buffer.  output_len=None: the decoded size is asked for first (cramjam_amd.batch.zstd_sizes)"""
    from . import _cramjam
    mv, exc = _view(data), _errors()[1]
    n, outs = _one(_N.ZSTD, _N.OP_DECOMPRESS, mv, _size(mv, exc) if output_len is None else int(output_len), None, exc)
    return _cramjam.Buffer(outs[0][:n])


def compress_into(input, output, level=None):
    """Compress directly into an output buffer; returns the frame's length.  `level`: as in compress"""
    _level(level)
    mv, exc = _view(input), _errors()[0]
    return _into(output, lambda out: _one(_N.ZSTD_COMPRESS, _N.OP_COMPRESS, mv, _bound(mv.nbytes, exc) if out is None else out.nbytes, out, exc))


def decompress_into(input, output):
    """Decompress directly into an output buffer; returns the decoded length"""
    mv, exc = _view(input), _errors()[1]
    return _into(output, lambda out: _one(_N.ZSTD, _N.OP_DECOMPRESS, mv, _size(mv, exc) if out is None else out.nbytes, out, exc))
