"""CPU model of Zlib and Zstd streams inside Blosc1 chunks (c-blosc 1.21, compressor formats 3 and 4): test infrastructure, not
product code.  The container is the one blosc_model walks; only the compressor format and the stream decoder differ:
  Zlib   Python's zlib.decompressobj: a stream is good iff it ends exactly at the stream's length and yields exactly dst_len bytes
  Zstd   libzstd's ZSTD_decompress through ctypes (tests/zstd_cases.libzstd): good iff it returns exactly dst_len
Also the loader of tests/golden/golden_blosc_zcodecs.json + .bin; the recorded verdicts and sha256 there need neither library."""
import ctypes as C
import hashlib
import json
import os
import struct
import zlib

import blosc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_BLOSCLZ, FLAG_ZLIB, FLAG_ZSTD = 2, 8, 16          # CJ_BLOSC_FLAG_READ_*
FLAGS = FLAG_ZLIB | FLAG_ZSTD
FORMAT_ZLIB, FORMAT_ZSTD = 3, 4
FLAG_OF = {FORMAT_ZLIB: FLAG_ZLIB, FORMAT_ZSTD: FLAG_ZSTD}


def fmt_of(chunk):
    """3 or 4 for a chunk whose streams are Zlib / Zstd: format 3 / 4, versionlz 1, not memcpyed; else None"""
    if len(chunk) >= 16 and chunk[0] == 2 and chunk[1] == 1 and chunk[2] >> 5 in FLAG_OF and not chunk[2] & 2:
        return chunk[2] >> 5
    return None


def zlib_stream(src, cap):
    d = zlib.decompressobj()
    try:
        out = d.decompress(bytes(src), cap + 1)          # (one byte more than fits: fewer came out only if the input or the stream ended)
    except zlib.error as ex:
        raise M.Refused(M.CORRUPT, "zlib: %s" % ex)
    if len(out) != cap or not d.eof or d.unused_data != b"":
        raise M.Refused(M.CORRUPT, "zlib: decoded %d of %d, eof %s, %d bytes behind the stream" % (len(out), cap, d.eof, len(d.unused_data)))
    return out


def zstd_stream(src, cap):
    import zstd_cases
    L = zstd_cases.libzstd()
    src = bytes(src)
    dst = C.create_string_buffer(max(cap, 1))
    r = L.ZSTD_decompress(dst, cap, src, len(src))
    if L.ZSTD_isError(r) or r != cap:
        raise M.Refused(M.CORRUPT, "zstd: %d of %d" % (-1 if L.ZSTD_isError(r) else r, cap))
    return dst.raw[:cap]


def decode_stream(fmt, src, cap):
    """the `cap` decoded bytes of one stream of compressor format fmt, or Refused(corrupt)"""
    return zlib_stream(src, cap) if fmt == FORMAT_ZLIB else zstd_stream(src, cap)


def parse(chunk, flags=FLAGS):
    """blosc_model.parse with the formats that `flags` ask for admitted: the format bits are rewritten for the parse only"""
    chunk = bytes(chunk)
    f = fmt_of(chunk)
    if f is None or not flags & FLAG_OF[f]:
        return M.parse(chunk)
    seen = bytearray(chunk)
    seen[2] = (seen[2] & 31) | (1 << 5)
    h, streams = M.parse(bytes(seen))
    h["flags"] = chunk[2]
    return h, streams


def decode(chunk, cap=None, flags=FLAGS):
    """the plain bytes of a chunk read with `flags`, or Refused (LZ4 chunks go to blosc_model.decode)"""
    chunk = bytes(chunk)
    f = fmt_of(chunk)
    if f is None or not flags & FLAG_OF[f]:
        return M.decode(chunk, cap)
    h, streams = parse(chunk, flags)
    n = h["nbytes"]
    if cap is not None and n > cap:
        raise M.Refused(M.TOO_SMALL)
    if n == 0:
        return b""
    image = bytearray(n)
    for src, ln, dst, dlen, _b, stored in streams:
        assert 16 <= src and src + ln <= len(chunk) and dst + dlen <= n
        image[dst:dst + dlen] = chunk[src:src + ln] if stored else decode_stream(f, chunk[src:src + ln], dlen)
    bs = h["blocksize"]
    out = bytearray()
    for at in range(0, n, bs):
        blk = image[at:at + bs]
        out += M.apply_filter(blk, h["typesize"], M.block_mode(h["flags"], h["typesize"], len(blk)), False)
    return bytes(out)


def verdict(chunk, cap=None, flags=FLAGS):
    try:
        return "ok", decode(chunk, cap, flags)
    except M.Refused as r:
        return r.cls, None


def wrap_one(fmt, stream, nbytes, extra=b""):
    """a chunk of one unsplit block of typesize 1 without a filter around `stream` + `extra`, the stream word counting both"""
    body = bytes(stream) + bytes(extra)
    assert len(body) != nbytes, "a stream of exactly its decoded length reads as stored"
    total = 16 + 4 + 4 + len(body)
    return struct.pack("<BBBBIII", 2, 1, 16 | (fmt << 5), 1, nbytes, nbytes, total) + struct.pack("<I", 20) + struct.pack("<i", len(body)) + body


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
_doc = None


def doc():
    global _doc
    if _doc is None:
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosc_zcodecs.json")) as f:
            _doc = json.load(f)
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosc_zcodecs.bin"), "rb") as f:
            blob = f.read()
        for i, v in enumerate(_doc["valid"]):
            v["name"] = M.name_of(v["recipe"], i)
            v["bytes"] = blob[v["at"]:v["at"] + v["len"]]
        for m in _doc["malformed"]:
            m["bytes"] = M.mutate(_doc["valid"][m["base"]]["bytes"], m["mutation"])
        for h in _doc["hand"]:
            h["bytes"] = blob[h["at"]:h["at"] + h["len"]]
    return _doc


def valid():
    return doc()["valid"]


def malformed():
    """seeded mutations inside stream payloads and of stream words, and the header cases; each with its recorded class"""
    return doc()["malformed"]


def hand():
    """the two hand-made chunks: a good stream followed by one extra byte that the stream word counts"""
    return doc()["hand"]


def make_input(kind, size, seed):
    """blosc_model.make_input, and one kind more: "f32lo", float32 values whose low mantissa byte is random and whose other bytes
    move slowly — behind the byte shuffle the first stream of a split block does not shrink and is stored, the other three do"""
    if kind != "f32lo":
        return M.make_input(kind, size, seed)
    import numpy as np
    rng = np.random.default_rng(seed)
    m = size // 4 + 1
    a = np.floor(np.arange(m, dtype=np.float64) / 64).astype(np.float32).view(np.uint32)
    a = (a & np.uint32(0xFFFFFF00)) | rng.integers(0, 256, m, dtype=np.uint32)
    return a.tobytes()[:size]


def raw_of(v):
    r = v["recipe"]
    return make_input(r["kind"], r["size"], r["seed"])


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def streams_of(chunk):
    """[(fmt, stream bytes, dst_len)] of the non-stored streams of a chunk of format 3 / 4 that parses, else []"""
    f = fmt_of(chunk)
    if f is None:
        return []
    try:
        return [(f, chunk[s:s + ln], dlen) for s, ln, _d, dlen, _b, st in parse(chunk)[1] if not st]
    except M.Refused:
        return []
