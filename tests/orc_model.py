"""The model of ORC compression streams, pure Python: the walk over the 3-byte chunk headers, frame() to build streams,
the verdict rules of cj_orc_batch_* given each chunk's size and decode result, the structural checks of what the encoder writes, and
the golden streams of tests/golden/golden_orc.* (pyarrow's ORC writer; make_golden_orc.py).  No CPU codec is needed at test time: the
chunks of the test cases come from the golden file, whose decoded bytes are recorded, or from Python's zlib."""
import hashlib
import json
import os
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = {"zlib": 1, "snappy": 2, "lz4": 4, "zstd": 5}          # ORC's CompressionKind
ORC_HEADER, ORC_BLOCK, OUT_TOO_SMALL, BAD_ARG, INPUT_TOO_LARGE = -60, -61, -6, -101, -1
CORRUPT = {"zlib": -40, "snappy": -12, "lz4": -7, "zstd": -51}  # the codec's "corrupt": a chunk that decodes to less than its size says
BLOCK_MAX, ENC_BLOCK_MAX = 1 << 23, 262144


def walk(s):
    """(code, [(offset of the chunk's bytes, their length, original)]): 0 or ORC_HEADER, the chunks before the error listed"""
    chunks, p, n = [], 0, len(s)
    while p < n:
        if n - p < 3:
            return ORC_HEADER, chunks
        h = s[p] | s[p + 1] << 8 | s[p + 2] << 16
        p += 3
        if (h >> 1) > n - p:
            return ORC_HEADER, chunks
        chunks.append((p, h >> 1, h & 1))
        p += h >> 1
    return 0, chunks


def header(length, original):
    assert 0 <= length < BLOCK_MAX
    return ((length << 1) | (1 if original else 0)).to_bytes(3, "little")


def frame(chunks):
    """the stream of (original, bytes) pairs"""
    return b"".join(header(len(c), o) + bytes(c) for o, c in chunks)


def compress_bound(n, block_size):
    if n > 0x7E000000 or not 1 <= block_size <= ENC_BLOCK_MAX:
        return 0
    return n + 3 * (-(-n // block_size))


def verdict(walk_code, sizes, block_size, cap=None, results=None):
    """The result of one stream.  sizes: per chunk in stream order its decoded size — an original's length, a compressed chunk's size-query
    answer (negative: the codec's code).  cap: the capacity (None: the size query).  results: per chunk the decode's result (None for an
    original chunk, or when every chunk decodes to its size).  Rules, in order: the walk's code; the first chunk in stream order whose
    size is an error or above block_size (ORC_BLOCK); OUT_TOO_SMALL when the sum exceeds cap; the first chunk in stream order whose
    decode result differs from its size (its code); else the sum."""
    if walk_code:
        return walk_code
    for v in sizes:
        if v < 0:
            return v
        if v > block_size:
            return ORC_BLOCK
    total = sum(sizes)
    if cap is not None and total > cap:
        return OUT_TOO_SMALL
    for v, r in zip(sizes, results or ()):
        if r is not None and r != v:
            assert r < 0
            return r
    return total


def check_encoded(s, raw, block_size, codec, random_input=False):
    """what the encoder's stream must look like, without decoding it: the walk accepts it; one chunk per piece of block_size bytes; an
    original chunk is its piece; a compressed chunk is shorter than its piece; nothing above the bound, and a stream of incompressible
    input is exactly the bound, all original.  Returns the chunks."""
    code, chunks = walk(s)
    assert code == 0
    pieces = [raw[i:i + block_size] for i in range(0, len(raw), block_size)]
    assert len(chunks) == len(pieces)
    for (off, n, orig), p in zip(chunks, pieces):
        if orig:
            assert bytes(s[off:off + n]) == bytes(p)
        else:
            assert 0 < n < len(p)
            if codec == "zlib":
                assert zlib.decompress(bytes(s[off:off + n]), -15) == bytes(p)
    assert len(s) <= compress_bound(len(raw), block_size)
    if random_input:
        assert len(s) == compress_bound(len(raw), block_size) and all(o for _, _, o in chunks)
    return chunks


def deflate_raw(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


# ---- the golden streams ------------------------------------------------------------------------------------------------------------------
_golden = None


def golden():
    """[{name, codec, block_size, stream (bytes), chunks [(off, len, original, decoded len, sha256 of the decoded bytes)], decoded_len, sha256}]"""
    global _golden
    if _golden is None:
        blob = open(os.path.join(GOLDEN, "golden_orc.bin"), "rb").read()
        recs = json.load(open(os.path.join(GOLDEN, "golden_orc.json")))["streams"]
        for r in recs:
            r["stream"] = blob[r["off"]:r["off"] + r["len"]]
            r["chunks"] = [tuple(c) for c in r["chunks"]]
        _golden = recs
    return _golden


def golden_of(codec, block_size=None):
    return [g for g in golden() if g["codec"] == codec and block_size in (None, g["block_size"])]


def digest(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def golden_chunks(codec, block_size=65536, original=False, min_decoded=0, max_decoded=1 << 30):
    """(chunk bytes, decoded length, SHA-256 of the decoded bytes) of the golden chunks of one codec that are compressed (original), by decoded length"""
    out = []
    for g in golden_of(codec, block_size):
        for off, n, orig, dlen, sha in g["chunks"]:
            if bool(orig) == original and min_decoded <= dlen <= max_decoded:
                out.append((g["stream"][off:off + n], dlen, sha))
    return out
