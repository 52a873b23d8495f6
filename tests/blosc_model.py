"""CPU model of the Blosc1 chunk format (c-blosc 1.x, format version 2, LZ4 streams): test infrastructure, not product code.
The decoder checks every bound itself and never reads outside the chunk; LZ4 blocks go through the oracle.  Also the seeded
input recipes that tests/golden/make_golden_blosc.py and the tests share (the fixtures store chunks, not their inputs)."""
import struct

import numpy as np

HEADER, UNSUPPORTED, CORRUPT, TOO_SMALL = "header", "unsupported", "corrupt", "too_small"
CODE = {HEADER: -30, UNSUPPORTED: -31, CORRUPT: -7, TOO_SMALL: -6}
CLASS = {v: k for k, v in CODE.items()}
MAX_BYTES = 0x7FFFFFFF - 16


class Refused(Exception):
    def __init__(self, cls, why=""):
        super().__init__("%s: %s" % (cls, why))
        self.cls = cls


def block_mode(flags, typesize, nbytes):
    """0 copy, 1 byte shuffle, 2 bitshuffle: what c-blosc does to a block of nbytes bytes"""
    if flags & 1 and typesize > 1:
        return 1
    if flags & 4 and nbytes >= typesize and (nbytes // typesize) % 8 == 0:
        return 2
    return 0


def shuffle(block, typesize):
    b = np.frombuffer(bytes(block), np.uint8)
    n = len(b) // typesize
    return np.ascontiguousarray(b[:n * typesize].reshape(n, typesize).T).tobytes() + b[n * typesize:].tobytes()


def unshuffle(block, typesize):
    b = np.frombuffer(bytes(block), np.uint8)
    n = len(b) // typesize
    return np.ascontiguousarray(b[:n * typesize].reshape(typesize, n).T).tobytes() + b[n * typesize:].tobytes()


def bitshuffle(block, typesize):
    """rows of the byte-shuffled image, each turned into 8 bit planes of n / 8 bytes (n a multiple of 8)"""
    b = np.frombuffer(bytes(block), np.uint8)
    n = len(b) // typesize
    assert n % 8 == 0
    rows = b[:n * typesize].reshape(n, typesize).T                                   # [typesize][n]
    bits = np.unpackbits(rows, axis=1, bitorder="little").reshape(typesize, n, 8)    # [j][i][plane]
    planes = np.packbits(bits.transpose(0, 2, 1), axis=2, bitorder="little")         # [j][plane][n / 8]
    return planes.tobytes() + b[n * typesize:].tobytes()


def bitunshuffle(block, typesize):
    b = np.frombuffer(bytes(block), np.uint8)
    n = len(b) // typesize
    assert n % 8 == 0
    planes = b[:n * typesize].reshape(typesize, 8, n // 8)
    bits = np.unpackbits(planes, axis=2, bitorder="little")                          # [j][plane][i]
    rows = np.packbits(bits.transpose(0, 2, 1), axis=2, bitorder="little").reshape(typesize, n)
    return np.ascontiguousarray(rows.T).tobytes() + b[n * typesize:].tobytes()


def apply_filter(block, typesize, mode, forward):
    if mode == 1:
        return (shuffle if forward else unshuffle)(block, typesize)
    if mode == 2:
        return (bitshuffle if forward else bitunshuffle)(block, typesize)
    return bytes(block)


def parse(chunk):
    """-> (header dict, streams): streams = [(src_off, src_len, dst_off, dst_len, block, stored)].  Raises Refused."""
    chunk = bytes(chunk)
    if len(chunk) < 16:
        raise Refused(HEADER, "short")
    version, versionlz, flags, typesize, nbytes, blocksize, cbytes = struct.unpack("<BBBBIII", chunk[:16])
    h = dict(version=version, versionlz=versionlz, flags=flags, typesize=typesize, nbytes=nbytes, blocksize=blocksize, cbytes=cbytes, nblocks=0)
    if version != 2:
        raise Refused(UNSUPPORTED, "format version")
    if flags & 8 or flags & 5 == 5:
        raise Refused(HEADER, "flags")
    if typesize == 0:
        raise Refused(HEADER, "typesize")
    if cbytes < 16 or cbytes > len(chunk):
        raise Refused(HEADER, "cbytes")
    if nbytes > MAX_BYTES:
        raise Refused(HEADER, "nbytes")
    if nbytes == 0:
        return h, []
    if blocksize == 0 or blocksize > nbytes:
        raise Refused(HEADER, "blocksize")
    if flags & 2:
        if cbytes != nbytes + 16:
            raise Refused(HEADER, "memcpyed size")
        return h, []
    if flags >> 5 != 1 or versionlz != 1:
        raise Refused(UNSUPPORTED, "compressor format")
    nblocks = (nbytes + blocksize - 1) // blocksize
    if 16 + 4 * nblocks > cbytes:
        raise Refused(HEADER, "block table")
    h["nblocks"] = nblocks
    streams = []
    leftover = nbytes % blocksize
    budget = cbytes // 5                     # streams that do not overlap take 5 bytes each at least
    for b in range(nblocks):
        short = leftover != 0 and b == nblocks - 1
        nb = leftover if short else blocksize
        nsplits = typesize if not flags & 16 and not short else 1
        if nb % nsplits or nsplits > budget:
            raise Refused(HEADER, "split")
        budget -= nsplits
        each = nb // nsplits
        pos = struct.unpack_from("<I", chunk, 16 + 4 * b)[0]
        if pos < 16 + 4 * nblocks:
            raise Refused(HEADER, "bstart")
        for k in range(nsplits):
            if pos + 4 > cbytes:
                raise Refused(HEADER, "stream word")
            cb = struct.unpack_from("<i", chunk, pos)[0]
            if cb <= 0 or pos + 4 + cb > cbytes:
                raise Refused(HEADER, "stream length")
            streams.append((pos + 4, cb, b * blocksize + k * each, each, b, cb == each))
            pos += 4 + cb
    return h, streams


def decode(chunk, cap=None):
    """the plain bytes, or Refused with the verdict class"""
    import oracle
    chunk = bytes(chunk)
    h, streams = parse(chunk)
    n = h["nbytes"]
    if cap is not None and n > cap:
        raise Refused(TOO_SMALL)
    if n == 0:
        return b""
    if h["flags"] & 2:
        return chunk[16:16 + n]
    image = bytearray(n)
    for src, ln, dst, dlen, _b, stored in streams:
        assert 16 <= src and src + ln <= len(chunk) and dst + dlen <= n
        if stored:
            image[dst:dst + dlen] = chunk[src:src + ln]
        else:
            r, out = oracle.lz4_decompress_raw(chunk[src:src + ln], dlen)
            if r != dlen:
                raise Refused(CORRUPT, "stream at %d: %d" % (src, r))
            image[dst:dst + dlen] = out
    bs = h["blocksize"]
    out = bytearray()
    for at in range(0, n, bs):
        blk = image[at:at + bs]
        out += apply_filter(blk, h["typesize"], block_mode(h["flags"], h["typesize"], len(blk)), False)
    return bytes(out)


def verdict(chunk, cap=None):
    """("ok", bytes) or (class, None)"""
    try:
        return "ok", decode(chunk, cap)
    except Refused as r:
        return r.cls, None


def mutate(chunk, mut):
    """a malformed fixture from its base chunk: ["cut", k] | ["put", offset, struct format, value] | ["swap", a, b, n]"""
    if mut[0] == "cut":
        return bytes(chunk[:mut[1]])
    b = bytearray(chunk)
    if mut[0] == "put":
        struct.pack_into(mut[2], b, mut[1], mut[3])
    else:
        _, x, y, n = mut
        b[x:x + n], b[y:y + n] = chunk[y:y + n], chunk[x:x + n]
    return bytes(b)


def name_of(r, i):
    """the name of valid fixture i from its recipe"""
    return "%03d_%s_t%d_s%d_f%d_c%d_%s_b%d_m%d" % (i, r["kind"], r["typesize"], r["size"], r["filter"], r["clevel"], r["cname"], r["blocksize"], r["split"])


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------
def make_input(kind, size, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return bytes(size)
    if kind == "rand":
        return rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    if kind == "text":
        phrase = bytes(rng.integers(97, 123, 97, dtype=np.uint8))
        a = np.frombuffer(phrase * (size // 97 + 1), np.uint8)[:size].copy()
        hits = rng.integers(0, max(size, 1), size // 8000 + 1)
        a[hits[hits < size]] = 32
        return a.tobytes()
    dt = {"f32": np.float32, "f64": np.float64, "i16": np.int16}[kind]
    item = np.dtype(dt).itemsize
    m = size // item + 1
    ramp = np.floor(np.arange(m, dtype=np.float64) / 64) + (rng.random(m) < 0.0005) * rng.integers(1, 1000, m)      # a ramp with sparse noise
    if kind == "i16":
        ramp = np.floor(ramp / 8) % 30000
    return ramp.astype(dt).tobytes()[:size]
