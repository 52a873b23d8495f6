"""Zstandard decode cases: the recorded fixtures (tests/golden/golden_zstd.*), the hand-written streams, a classifier of frames by
their block and section headers and a deeper one that reads table and tree descriptions and the sequences' codes (deep_classify: the
reader that checks what tests/zstd_synth.py claims to write), libzstd through ctypes (the reference of every verdict; CPU tests only)
and a scalar XXH64."""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import random
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_JSON = os.path.join(HERE, "golden", "golden_zstd.json")
GOLDEN_BIN = os.path.join(HERE, "golden", "golden_zstd.bin")

E_OUT_TOO_SMALL, E_HEADER, E_CORRUPT, E_CHECKSUM, E_SRC_SIZE, E_DICT = -6, -50, -51, -52, -53, -54
# libzstd's ZSTD_ErrorCode -> the CJ_E_* family (include/cramjam_hip.h); 30 = dictionary_corrupted (Treeless literals without a table)
ERROR_FAMILY = {10: E_HEADER, 14: E_HEADER, 16: E_HEADER, 20: E_CORRUPT, 30: E_CORRUPT, 22: E_CHECKSUM, 72: E_SRC_SIZE, 32: E_DICT, 70: E_OUT_TOO_SMALL}

# Cases where the decoder deliberately differs from libzstd: {case name: reason}.  At most 2 % of all cases.
DIVERGES_FROM_ZSTD = {
    "legacy_v07": "a libzstd built with legacy support reads v0.7 frames; legacy frames are out of scope and refused as a bad magic (CJ_E_ZSTD_HEADER)",
}

# every mode a fixture set has to show (make_golden_zstd.py and test_zstd_model.py assert it)
COVERAGE = ["block:raw", "block:rle", "block:compressed", "lit:raw", "lit:rle", "lit:huf1", "lit:huf4", "lit:treeless",
            "weights:direct", "weights:fse", "nseq:0", "nseq:1byte", "nseq:2byte", "nseq:3byte",
            "ll:predefined", "ll:rle", "ll:fse", "ll:repeat", "of:predefined", "of:rle", "of:fse", "of:repeat",
            "ml:predefined", "ml:rle", "ml:fse", "ml:repeat", "frame:checksum", "frame:nochecksum", "frame:fcs", "frame:nofcs",
            "frame:single", "frame:window", "chunk:multiframe", "chunk:skippable", "chunk:empty"]


# ---- libzstd ------------------------------------------------------------------------------------------------------------------------
_zstd = None


def _libzstd_file():
    """The system's libzstd by its FILE.  By its soname, dlopen hands back whichever libzstd.so.1 the process already holds: behind a
    libblosc that brings a libzstd of its own (one built without the legacy formats answers -50 on a v0.7 frame where the fixtures'
    libzstd answers -53) the reference would silently be another library, and the fixtures would depend on the order of the tests."""
    import subprocess
    name = ctypes.util.find_library("zstd") or "libzstd.so.1"
    try:
        cache = subprocess.run(["/sbin/ldconfig", "-p"], capture_output=True, text=True).stdout
    except OSError:
        return name
    for line in cache.splitlines():
        if line.strip().startswith(name + " ") and "=>" in line:
            return line.split("=>")[1].strip()
    return name


def libzstd():
    global _zstd
    if _zstd is None:
        L = C.CDLL(_libzstd_file(), mode=os.RTLD_NOW | getattr(os, "RTLD_DEEPBIND", 0))
        L.ZSTD_decompress.restype = C.c_size_t
        L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.ZSTD_compress2.restype = C.c_size_t
        L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.ZSTD_compressBound.restype = C.c_size_t
        L.ZSTD_compressBound.argtypes = [C.c_size_t]
        L.ZSTD_createCCtx.restype = C.c_void_p
        L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        L.ZSTD_CCtx_setParameter.restype = C.c_size_t
        L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ZSTD_isError.argtypes = [C.c_size_t]
        L.ZSTD_getErrorCode.argtypes = [C.c_size_t]
        L.ZSTD_versionString.restype = C.c_char_p
        _zstd = L
    return _zstd


PARAMS = {"level": 100, "windowLog": 101, "hashLog": 102, "chainLog": 103, "searchLog": 104, "minMatch": 105, "targetLength": 106,
          "strategy": 107, "contentSize": 200, "checksum": 201, "targetCBlockSize": 1003}


def zstd_compress(data, **params):
    L = libzstd()
    cctx = L.ZSTD_createCCtx()
    try:
        for k, v in params.items():
            rc = L.ZSTD_CCtx_setParameter(cctx, PARAMS[k], v)
            if L.ZSTD_isError(rc):
                raise ValueError("libzstd refuses %s=%r" % (k, v))
        cap = L.ZSTD_compressBound(len(data))
        out = C.create_string_buffer(cap)
        n = L.ZSTD_compress2(cctx, out, cap, bytes(data), len(data))
        assert not L.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        L.ZSTD_freeCCtx(cctx)


def zstd_verdict(stream, cap):
    """(result as the C-ABI states it, output bytes) of ZSTD_decompress(dst, cap, stream, len(stream))"""
    L = libzstd()
    out = C.create_string_buffer(cap + 1)
    r = L.ZSTD_decompress(out, cap, bytes(stream), len(stream))
    if L.ZSTD_isError(r):
        return ERROR_FAMILY[L.ZSTD_getErrorCode(r)], b""
    return int(r), out.raw[:r]


# ---- a scalar XXH64 --------------------------------------------------------------------------------------------------------------------
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(data, seed=0):
    data = bytes(data)
    n, at = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while at + 32 <= n:
            for j, w in enumerate(struct.unpack_from("<4Q", data, at)):
                v[j] = _round(v[j], w)
            at += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for x in v:
            h = ((h ^ _round(0, x)) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while at + 8 <= n:
        h ^= _round(0, struct.unpack_from("<Q", data, at)[0])
        h = (_rotl(h, 27) * _P1 + _P4) & _M
        at += 8
    if at + 4 <= n:
        h ^= (struct.unpack_from("<I", data, at)[0] * _P1) & _M
        h = (_rotl(h, 23) * _P2 + _P3) & _M
        at += 4
    while at < n:
        h ^= (data[at] * _P5) & _M
        h = (_rotl(h, 11) * _P1) & _M
        at += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)


# ---- a small frame writer: what libzstd never writes ----------------------------------------------------------------------------------
def backward_bits(fields):
    """the bytes of a backward bitstream whose reader meets `fields` = [(value, nbits), ...] in this order; final-bit marker on top"""
    acc, total = 1, 0
    for v, nb in fields:
        assert 0 <= v < (1 << nb) or nb == 0
        acc = (acc << nb) | v
        total += nb
    return acc.to_bytes((total + 1 + 7) // 8, "little")


def literals_header(kind, size):
    if size < 32:
        return bytes([(size << 3) | kind])
    if size < 4096:
        return struct.pack("<H", (size << 4) | (1 << 2) | kind)
    return struct.pack("<I", (size << 4) | (3 << 2) | kind)[:3]


def nseq_bytes(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([0x80 + (n >> 8), n & 255])
    return b"\xff" + struct.pack("<H", n - 0x7F00)


def rle_sequences(n, ll_code, of_code, ml_code, extras=()):
    """a sequences section of n sequences, RLE mode on all three codes; extras: per sequence (of, ml, ll) extra-bit fields"""
    fields = []
    for e in extras:
        fields += list(e)
    return nseq_bytes(n) + bytes([0x54, ll_code, of_code, ml_code]) + backward_bits(fields)


def block(kind, last, payload, size=None):
    size = len(payload) if size is None else size
    return struct.pack("<I", (size << 3) | (kind << 1) | (1 if last else 0))[:3] + payload


def frame(blocks, content=None, checksum=False, fcs=False):
    fhd = (4 if checksum else 0) | (0x80 if fcs else 0)
    out = b"\x28\xb5\x2f\xfd" + bytes([fhd, 0x58]) + (struct.pack("<I", len(content)) if fcs else b"") + b"".join(blocks)
    return out + (struct.pack("<I", xxh64(content) & 0xFFFFFFFF) if checksum else b"")


def hand_streams():
    """{name: (stream, the bytes it decodes to)}"""
    out = {}
    for n in (127, 128, 0x7EFF, 0x7F00):                      # the sequence count's three widths: literal 'k', then 3 bytes at offset 1
        rnd = random.Random(n)
        lits = bytes(rnd.randrange(256) for _ in range(n))
        body = literals_header(0, n) + lits + rle_sequences(n, 1, 0, 0)
        data = b"".join(bytes([b]) * 4 for b in lits)
        out["hand_nseq_%d" % n] = (frame([block(2, True, body)], data, checksum=True, fcs=(n & 1) == 0), data)
    # RLE literals, an RLE block, a block of 0 sequences, Repeat on all three codes behind an RLE-mode block
    b1 = literals_header(1, 40) + b"Z" + rle_sequences(3, 2, 0, 1)                        # 3 x (2 literals, 4 bytes at offset 1)
    b2 = literals_header(0, 5) + b"hello" + bytes([0])                                    # no sequences
    b3 = literals_header(0, 9) + b"ABCDEFGHI" + nseq_bytes(3) + bytes([0xFC]) + backward_bits([])      # Repeat x 3
    data = b"Z" * 18 + b"Z" * 34 + b"Q" * 1000 + b"hello" + b"ABBBBBCDDDDDEFFFFFGHI"
    out["hand_rle_repeat"] = (frame([block(2, False, b1), block(1, False, b"Q", 1000), block(2, False, b2), block(2, True, b3)], data, checksum=True), data)
    # a match that reaches back into the previous block (offset 16 = code 4, extra 3), then the repeat offset carried into the next block
    raw = bytes(range(65, 81))
    b2 = literals_header(0, 0) + rle_sequences(1, 0, 4, 0, [((3, 4), (0, 0), (0, 0))])
    b3 = literals_header(0, 1) + b"!" + rle_sequences(1, 1, 0, 2)                          # 1 literal, 5 bytes at the repeat offset (16)
    data = raw + raw[:3] + b"!" + (raw + raw[:3] + b"!")[-16:][:5]
    out["hand_cross_block"] = (frame([block(0, False, raw), block(2, False, b2), block(2, True, b3)], data, checksum=True, fcs=True), data)
    # Treeless literals and a Repeat table before anything could be repeated: refused
    out["hand_repeat_first"] = (frame([block(2, True, literals_header(0, 1) + b"x" + nseq_bytes(1) + bytes([0xFC]) + b"\x01")]), None)
    out["hand_treeless_first"] = (frame([block(2, True, struct.pack("<I", 3 | (4 << 4) | (2 << 14))[:3] + b"\x01\x01" + bytes([0]))]), None)
    out["hand_reserved_block"] = (frame([block(3, True, b"abc")]), None)
    # frames WITHOUT a content size whose sequences break a rule the size query still checks: an offset beyond the frame's output
    # (16 behind 4 bytes) and a literal length beyond the block's literals (2 of 1)
    out["hand_bad_offset"] = (frame([block(0, False, b"abcd"), block(2, True, literals_header(0, 0) + rle_sequences(1, 0, 4, 0, [((3, 4), (0, 0), (0, 0))]))]), None)
    out["hand_literal_overrun"] = (frame([block(0, False, b"abcd"), block(2, True, literals_header(0, 1) + b"x" + rle_sequences(1, 2, 0, 0))]), None)
    return out


# ---- the classifier: the modes a chunk shows, from its block and section headers ------------------------------------------------------
def classify(stream):
    tags, ip, n, frames = set(), 0, len(stream), 0
    if n == 0:
        tags.add("chunk:empty")
    while n - ip >= 8:
        magic = struct.unpack_from("<I", stream, ip)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            tags.add("chunk:skippable")
            ip += 8 + struct.unpack_from("<I", stream, ip + 4)[0]
            continue
        assert magic == 0xFD2FB528
        frames += 1
        fhd = stream[ip + 4]
        single, fcs_code, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
        fcs_len = (1 << fcs_code) if fcs_code else single
        tags.add("frame:checksum" if fhd & 4 else "frame:nochecksum")
        tags.add("frame:fcs" if fcs_len else "frame:nofcs")
        tags.add("frame:single" if single else "frame:window")
        ip += 5 + (0 if single else 1) + (4 if did == 3 else did) + fcs_len
        huf_seen = False
        while True:
            bh = stream[ip] | (stream[ip + 1] << 8) | (stream[ip + 2] << 16)
            last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
            ip += 3
            tags.add("block:" + ("raw", "rle", "compressed")[kind])
            if kind == 2:
                q, b0 = ip, stream[ip]
                lk, lhl = b0 & 3, (b0 >> 2) & 3
                if lk < 2:
                    lh = (1, 2, 1, 3)[lhl]
                    lsize = int.from_bytes(stream[q:q + lh], "little") >> (3 if lh == 1 else 4)
                    tags.add("lit:raw" if lk == 0 else "lit:rle")
                    q += lh + (lsize if lk == 0 else 1)
                else:
                    lh = (3, 3, 4, 5)[lhl]
                    v = int.from_bytes(stream[q:q + lh], "little")
                    bits = (10, 10, 14, 18)[lhl]
                    lcs = (v >> (4 + bits)) & ((1 << bits) - 1)
                    tags.add("lit:huf1" if lhl == 0 else "lit:huf4")
                    if lk == 3:
                        tags.add("lit:treeless")
                    else:
                        tags.add("weights:direct" if stream[q + lh] >= 128 else "weights:fse")
                    q += lh + lcs
                ns = stream[q]
                if ns == 0:
                    tags.add("nseq:0")
                else:
                    width = 1 if ns < 128 else 3 if ns == 255 else 2
                    tags.add("nseq:%dbyte" % width)
                    modes = stream[q + width]
                    for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
                        tags.add("%s:%s" % (name, ("predefined", "rle", "fse", "repeat")[(modes >> sh) & 3]))
            ip += 1 if kind == 1 else size
            if last:
                break
        ip += 4 if fhd & 4 else 0
    if frames > 1:
        tags.add("chunk:multiframe")
    return tags


# ---- a second reader, not the writer of zstd_synth.py: the grammar corners a chunk shows ------------------------------------------------
# every corner a synthesized set has to show (test_zstd_synth_model.py asserts it)
DEEP_COVERAGE = (["%s:log%d" % (c, k) for c, top in (("ll", 9), ("of", 8), ("ml", 9), ("w", 6)) for k in range(5, top + 1)]
                 + ["nc:less_than_one", "nc:run0", "nc:run1", "nc:run2", "nc:run3chain", "nc:run12", "nc:short", "nc:long_low", "nc:long_high",
                    "nc:under8", "nc:tail", "nc:block_end"]
                 + ["huf:log%d" % k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)] + ["huf:last%d" % k for k in range(1, 13)] + ["huf:2symbols", "huf:256symbols", "huf:sym255", "huf:128direct"]
                 + ["weights:direct", "weights:fse", "lit:huf1", "lit:huf4", "lit:treeless"]
                 + ["lh:huf%d" % k for k in range(4)] + ["lh:treeless%d" % k for k in range(4)] + ["lh:raw%d" % k for k in range(4)] + ["lh:rle%d" % k for k in range(4)]
                 + ["off:new", "off:rep1", "off:rep2", "off:rep3", "off:ll0_rep2", "off:ll0_rep3", "off:ll0_rep1m1", "off:forced1", "seq:reload31",
                    "seq:bits30", "seq:bits31", "seq:bits32", "seq:prefetch", "seq:leftover_bits"]
                 + ["%s:%s>%s" % (c, a, b) for c in ("ll", "of", "ml") for a in ("predefined", "rle", "fse", "repeat") for b in ("predefined", "rle", "fse", "repeat")]
                 + ["fcs:1", "fcs:2", "fcs:4", "fcs:8", "frame:single", "frame:window", "wd:0x00", "wd:0xa8", "chunk:skippable0", "chunk:8frames",
                    "block:empty_raw", "block:empty_rle"])


class _Fwd:
    """a forward bit reader, least significant bit first"""
    def __init__(self, data):
        self.v, self.n, self.at = int.from_bytes(data, "little"), 8 * len(data), 0

    def peek(self, nb):
        return (self.v >> self.at) & ((1 << nb) - 1)

    def read(self, nb):
        v = self.peek(nb)
        self.at += nb
        return v


class _Bwd:
    """a backward bit reader: bits behind the stream's start read as 0, `left` goes negative"""
    def __init__(self, data):
        assert data and data[-1]
        self.v = int.from_bytes(data, "little")
        self.left = self.v.bit_length() - 1

    def read(self, nb):
        self.left -= nb
        return ((self.v >> self.left) if self.left >= 0 else (self.v << -self.left)) & ((1 << nb) - 1)


def read_ncount(data, max_sv, tags):
    """RFC 8878 4.1.1 over data (everything the description may use): (log, counts, bytes used); tags gets the forms met"""
    b = _Fwd(data)
    log = b.read(4) + 5
    remaining, counts = (1 << log) + 1, []
    if len(data) < 8:
        tags.add("nc:under8")
    while remaining > 1 and len(counts) <= max_sv:
        if len(data) >= 8 and b.at // 8 > len(data) - 4:
            tags.add("nc:tail")
        nb = remaining.bit_length()                          # bits of the largest value, `remaining`
        low = (1 << nb) - 1 - remaining                      # values below it take one bit less
        v = b.peek(nb - 1)
        if v < low:
            b.read(nb - 1)
            tags.add("nc:short")
        else:
            v = b.read(nb)
            tags.add("nc:long_high" if v >= (1 << (nb - 1)) else "nc:long_low")
            if v >= (1 << (nb - 1)):
                v -= low
        c = v - 1
        counts.append(c)
        remaining -= abs(c)
        if c == -1:
            tags.add("nc:less_than_one")
        if c == 0:
            run = 0
            while True:
                r = b.read(2)
                counts += [0] * r
                if r < 3:
                    tags.add("nc:run%d" % r if run == 0 else "nc:run3chain")
                    break
                run += 1
            if run >= 12:
                tags.add("nc:run12")
    assert remaining == 1 and len(counts) <= max_sv + 1 and (b.at + 7) // 8 <= len(data)
    return log, counts, (b.at + 7) // 8


def fse_cells(log, counts):
    """RFC 8878 4.1.1: per cell (symbol, bits, base)"""
    size = 1 << log
    cell, top = [None] * size, size
    for s, c in enumerate(counts):
        if c == -1:
            top -= 1
            cell[top] = s
    at = 0
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            cell[at] = s
            at = (at + (size >> 1) + (size >> 3) + 3) % size
            while at >= top:
                at = (at + (size >> 1) + (size >> 3) + 3) % size
    seen, out = [abs(c) for c in counts], []
    for s in cell:
        x = seen[s]
        seen[s] += 1
        nb = log - (x.bit_length() - 1)
        out.append((s, nb, (x << nb) - size))
    return out


_LLB = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
_MLB = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
_LLV = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
_DEFAULTS = {"ll": (6, [4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]),
             "of": (5, [1] * 6 + [2, 2, 2] + [1] * 15 + [-1] * 5),
             "ml": (6, [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7)}


def deep_classify(stream):
    """classify() and the corners of DEEP_COVERAGE, by decoding table descriptions, tree descriptions and the sequences' codes; a
    chunk that breaks the grammar yields what was met before the break"""
    tags = set()
    try:
        _deep(bytes(stream), tags)
    except (AssertionError, IndexError, struct.error, ValueError, StopIteration):
        pass
    return tags


def _deep(s, tags):
    ip, frames, skip0 = 0, 0, False
    while len(s) - ip >= 8:
        if struct.unpack_from("<I", s, ip)[0] & 0xFFFFFFF0 == 0x184D2A50:
            size = struct.unpack_from("<I", s, ip + 4)[0]
            tags.add("chunk:skippable")
            if size == 0:
                tags.add("chunk:skippable0")
            ip += 8 + size
            continue
        assert s[ip:ip + 4] == b"\x28\xb5\x2f\xfd"
        frames += 1
        if frames == 8:
            tags.add("chunk:8frames")
        fhd = s[ip + 4]
        single, code = (fhd >> 5) & 1, fhd >> 6
        assert not fhd & 8 and not fhd & 3
        fcs_len = (1 << code) if code else single
        tags.add("frame:single" if single else "frame:window")
        window = 0
        if not single:
            tags.add("wd:0x%02x" % s[ip + 5])
            window = (8 + (s[ip + 5] & 7)) << (7 + (s[ip + 5] >> 3))
        if fcs_len:
            tags.add("fcs:%d" % fcs_len)
        ip += 5 + (0 if single else 1) + fcs_len
        tabs, prev, reps, produced = {}, {}, [1, 4, 8], 0
        while True:
            bh = int.from_bytes(s[ip:ip + 3], "little")
            last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
            ip += 3
            assert kind < 3
            if last and size == 0:
                tags.add("block:empty_" + ("raw", "rle", "compressed")[kind])
            if kind < 2:
                produced += size
                ip += size if kind == 0 else 1
            else:
                end = ip + size
                assert end <= len(s)
                b0 = s[ip]
                lk, lhl = b0 & 3, (b0 >> 2) & 3
                if lk < 2:
                    lh = (1, 2, 1, 3)[lhl]
                    nlit = int.from_bytes(s[ip:ip + lh], "little") >> (3 if lh == 1 else 4)
                    tags.add("lh:%s%d" % (("raw", "rle")[lk], lhl))
                    q = ip + lh + (nlit if lk == 0 else 1)
                else:
                    lh, nb = (3, 3, 4, 5)[lhl], (10, 10, 14, 18)[lhl]
                    v = int.from_bytes(s[ip:ip + lh], "little")
                    nlit, lcs = (v >> 4) & ((1 << nb) - 1), (v >> (4 + nb)) & ((1 << nb) - 1)
                    tags.add("lh:%s%d" % (("huf", "treeless")[lk - 2], lhl))
                    q = ip + lh + lcs
                    assert q <= end
                    if lk == 2:
                        _deep_tree(s[ip + lh:q], tags)
                    tags.add("lit:treeless" if lk == 3 else "lit:huf1" if lhl == 0 else "lit:huf4")
                nseq = s[q]
                q += 1
                if nseq >= 128:
                    nseq = (s[q] | (s[q + 1] << 8)) + 0x7F00 if nseq == 255 else ((nseq - 128) << 8) + s[q]
                    q += 2 if s[q - 1] == 255 else 1
                if nseq:
                    modes = s[q]
                    q += 1
                    for name, sh, max_sv in (("ll", 6, 35), ("of", 4, 31), ("ml", 2, 52)):
                        m = (modes >> sh) & 3
                        mname = ("predefined", "rle", "fse", "repeat")[m]
                        if name in prev:
                            tags.add("%s:%s>%s" % (name, prev[name], mname))
                        prev[name] = mname
                        if m == 0:
                            tabs[name] = (_DEFAULTS[name][0], fse_cells(*_DEFAULTS[name]))
                        elif m == 1:
                            tabs[name] = (0, [(s[q], 0, 0)])
                            q += 1
                        elif m == 2:
                            sub = set()
                            log, counts, used = read_ncount(s[q:end], max_sv, sub)
                            if q + used == end:
                                sub.add("nc:block_end")
                            tags |= sub
                            tags.add("%s:log%d" % (name, log))
                            tabs[name] = (log, fse_cells(log, counts))
                            q += used
                        else:
                            assert name in tabs
                    b = _Bwd(s[q:end])
                    st = {k: b.read(tabs[k][0]) for k in ("ll", "of", "ml")}
                    for i in range(nseq):
                        cl, co, cm = (tabs[k][1][st[k]] for k in ("ll", "of", "ml"))
                        extra = b.read(co[0])
                        b.read(_MLB[cm[0]])
                        ll = _LLV[cl[0]] + b.read(_LLB[cl[0]])
                        total = co[0] + _MLB[cm[0]] + _LLB[cl[0]]
                        if total >= 31:
                            tags.add("seq:reload31")
                        if 30 <= total <= 32:
                            tags.add("seq:bits%d" % total)
                        if co[0] > 1:
                            tags.add("off:new")
                            reps = [(1 << co[0]) + extra - 3, reps[0], reps[1]]
                        else:
                            k = co[0] + extra + (ll == 0)               # 0: the first repeat offset ... 3: that minus one
                            tags.add(("off:rep1", "off:ll0_rep2" if ll == 0 else "off:rep2", "off:ll0_rep3" if ll == 0 else "off:rep3", "off:ll0_rep1m1")[k])
                            if k:
                                t = reps[k] if k < 3 else reps[0] - 1
                                if t == 0:
                                    tags.add("off:forced1")
                                    t = 1
                                reps = [t, reps[0], reps[1]] if k > 1 else [t, reps[0], reps[2]]
                        if i + 1 < nseq:
                            for k, c in (("ll", cl), ("ml", cm), ("of", co)):
                                st[k] = c[2] + b.read(c[1])
                    # libzstd's prefetching decoder (a window above 16 MiB, over 4 sequences, offset cells above 22 bits) takes leftovers
                    far = sum(1 for c in tabs["of"][1] if c[0] > 22) << (8 - tabs["of"][0])
                    if window > (1 << 24) and nseq > 4 and far >= 7:
                        tags.add("seq:prefetch")
                        if b.left > 0:
                            tags.add("seq:leftover_bits")
                    else:
                        assert b.left == 0
                ip = end
            if last:
                break
        ip += 4 if fhd & 4 else 0


def _deep_tree(d, tags):
    """a Huffman tree description at the head of d"""
    if d[0] >= 128:
        n = d[0] - 127
        w = [(d[1 + k // 2] >> (0 if k & 1 else 4)) & 15 for k in range(n)]
        tags.add("weights:direct")
        if n == 128:
            tags.add("huf:128direct")
    else:
        sub = set()
        log, counts, used = read_ncount(d[1:1 + d[0]], 255, sub)
        cells = fse_cells(log, counts)
        b = _Bwd(d[1 + used:1 + d[0]])
        st, w, k = [b.read(log), b.read(log)], [], 0
        while len(w) < 256:
            c = cells[st[k]]
            w.append(c[0])
            st[k] = c[2] + b.read(c[1])
            if b.left < 0:
                w.append(cells[st[k ^ 1]][0])
                break
            k ^= 1
        tags |= sub
        tags.add("weights:fse")
        tags.add("w:log%d" % log)
        tags.add("w:%dsymbols" % len(counts))
    total = sum(1 << (x - 1) for x in w if x)
    hlog = total.bit_length()
    rest = (1 << hlog) - total
    assert rest & (rest - 1) == 0 and rest and max(w) < 12
    tags.add("huf:log%d" % hlog)
    tags.add("huf:last%d" % rest.bit_length())                # the implied last weight
    nsym = sum(1 for x in w if x) + 1
    if nsym == 2:
        tags.add("huf:2symbols")
    if nsym == 256:
        tags.add("huf:256symbols")
    if len(w) == 255:
        tags.add("huf:sym255")


def huffman_literals_before_failure(stream):
    """True when a walk of the chunk's headers meets a block with Huffman or Treeless literals (before whatever makes the walk of a
    damaged chunk fail): the blocks whose errors only decoding the literals can find"""
    ip, n = 0, len(stream)
    try:
        while n - ip >= 8:
            magic = struct.unpack_from("<I", stream, ip)[0]
            if magic & 0xFFFFFFF0 == 0x184D2A50:
                ip += 8 + struct.unpack_from("<I", stream, ip + 4)[0]
                continue
            fhd = stream[ip + 4]
            single, fcs_code, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
            ip += 5 + (0 if single else 1) + (4 if did == 3 else did) + ((1 << fcs_code) if fcs_code else single)
            while True:
                bh = stream[ip] | (stream[ip + 1] << 8) | (stream[ip + 2] << 16)
                ip += 3
                if (bh >> 1) & 3 == 2 and stream[ip] & 3 >= 2:
                    return True
                ip += 1 if (bh >> 1) & 3 == 1 else bh >> 3
                if bh & 1:
                    break
            ip += 4 if fhd & 4 else 0
    except (IndexError, struct.error):
        pass
    return False


def any_frame_has_content_size(stream):
    """True when the first frame header of the chunk carries Frame_Content_Size (mutations keep the frame layout of their base)"""
    return len(stream) >= 5 and stream[:4] == b"\x28\xb5\x2f\xfd" and ((stream[4] >> 6) != 0 or bool((stream[4] >> 5) & 1))


def size_query_may_miss(stream, d):
    """the statement of zstd_wave.hpp / cramjam_hip.h: may the size query answer something else than the decoder's error d?"""
    if d == E_CHECKSUM:
        return True
    if any_frame_has_content_size(stream):                      # block bodies are skipped
        return d in (E_CORRUPT, E_SRC_SIZE)
    return d == E_CORRUPT and huffman_literals_before_failure(stream)      # only the literals' decoding finds it


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------
def mutate(base, seed):
    """one seeded mutation of a stream: a flipped bit, a changed byte, a cut tail, a dropped or a doubled byte"""
    rnd = random.Random(seed)
    b = bytearray(base)
    how = rnd.randrange(10)
    at = rnd.randrange(len(b))
    if how < 4:
        b[at] ^= 1 << rnd.randrange(8)
    elif how < 7:
        b[at] = rnd.randrange(256)
    elif how == 7:
        del b[max(1, at):]
    elif how == 8:
        del b[at]
    else:
        b.insert(at, b[at])
    return bytes(b)


# ---- the recorded fixtures -----------------------------------------------------------------------------------------------------------
def capacities(cap):
    return [cap, cap + 64, max(cap - 1, 0), 0]


class Case:
    def __init__(self, name, stream, cap, verdicts, sha, tags):
        self.name, self.stream, self.cap, self.verdicts, self.sha, self.tags = name, stream, cap, verdicts, sha, tags

    @property
    def accepted(self):
        return self.verdicts[0] >= 0


_cases = None


def load_cases():
    """every recorded case: fixtures, hand-written streams and mutations (stored as edits of their base stream's bytes)"""
    global _cases
    if _cases is None:
        meta = json.load(open(GOLDEN_JSON))
        blob = open(GOLDEN_BIN, "rb").read()
        _cases, by = [], {}
        for m in meta["cases"]:
            if "base" in m:                                  # a mutation: the base's first `pre` and last `suf` bytes around `mid`
                b = by[m["base"]]
                s = b[:m["pre"]] + bytes.fromhex(m["mid"]) + b[len(b) - m["suf"]:]
            else:
                s = by[m["name"]] = blob[m["off"]:m["off"] + m["len"]]
            _cases.append(Case(m["name"], s, m["cap"], m["verdicts"], m["sha"], set(m["tags"])))
    return _cases


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def device_call(e, N, chunks, caps, sizes=False):
    """cj_zstd_batch_device (sizes: cj_zstd_batch_sizes_device) in the harness's guarded run (tests/device_batch.py): chunks at every
    misalignment, 64 guard bytes around every slot, the output filled with 0xA5 first: (results, output, offsets)"""
    import device_batch as DB
    n, L = len(chunks), N.lib()
    if sizes:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_sizes_device(e.h, N.ZSTD_FRAMES, 0, n, i, o, l, r, None))
    else:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, n, i, o, l, out, oo, oc, r, None))
    return DB.run_chunks(e, call, chunks, caps)


def check_batch(part, which, res, out, ooff, caps, digest=sha):
    """every chunk of a device_call against verdict `which`: the result, both guards, [result, cap) untouched, at the exact capacity the bytes' digest"""
    from device_batch import G
    for i, c in enumerate(part):
        want = c.verdicts[which]
        assert res[i] == want, (c.name, caps[i], int(res[i]), want)
        lo, cap = ooff[i], int(caps[i])
        assert (out[lo - G:lo] == 0xA5).all() and (out[lo + cap:lo + cap + G] == 0xA5).all(), c.name
        if want >= 0:
            assert (out[lo + want:lo + cap] == 0xA5).all(), c.name        # bytes between the result and the capacity stay untouched
            if which == 0:
                assert digest(out[lo:lo + want]) == c.sha, c.name
