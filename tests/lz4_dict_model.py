"""LZ4 blocks written against a shared dictionary (LZ4_loadDict + LZ4_compress_fast_continue, read by LZ4_decompress_safe_usingDict):
the Python model of the decode rules and of the size walk that cramjam_amd/csrc/lz4_wave.hpp (kDict = true) and lz4_size_walk.hpp implement,
the seeded inputs of the fixtures, the hand-written edge streams, and the loader of tests/golden/golden_dict.json / .bin (minted by
tests/golden/make_golden_dict.py from the system liblz4).  No GPU, no liblz4 needed to import it."""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CORRUPT, NO_PREFIX, NEG_PREFIX, PREFIX_TOO_BIG, OUT_TOO_SMALL, INPUT_TOO_LARGE, BAD_ARG = -7, -3, -4, -5, -6, -1, -101
WINDOW = 65536
DICT_LENS = (1, 7, 4096, 65535, 65536, 70000)
BATCH_DICT_LENS = DICT_LENS + (65534,)      # ... and the one further length a hand-written stream needs: the batches of the tests
RECORD_SIZES = (0, 1, 12, 13, 64, 300, 4096, 16384, 65536, 70000, 200000)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def _vocabulary(seed=2024, words=600):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(words):
        k = int(rng.integers(2, 11))
        out.append(bytes(rng.integers(97, 123, k, dtype=np.uint8)))
    return out


_VOCAB = _vocabulary()


def words(size, seed, pool=None):
    """`size` bytes of space-separated words of the vocabulary (pool: only its first `pool` words)"""
    rng = np.random.default_rng(seed)
    v = _VOCAB if pool is None else _VOCAB[:pool]
    out = bytearray()
    while len(out) < size:
        idx = rng.integers(0, len(v), 256)
        out += b" ".join(v[i] for i in idx) + b" "
    return bytes(out[:size])


def dict_buffer():
    """the one seeded 70 000-byte buffer the fixtures' dictionaries are tails of"""
    return words(70000, 1)


def dictionary(length):
    b = dict_buffer()
    return b[len(b) - length:]


def record(size, seed):
    """a compressible record: phrases of the vocabulary drawn from a small pool, so that the fixture file stays small"""
    rng = np.random.default_rng(1000 + seed)
    phrases = [words(int(rng.integers(12, 60)), 5000 + seed * 97 + k) for k in range(48)]
    out = bytearray()
    while len(out) < size:
        out += phrases[int(rng.integers(0, len(phrases)))]
    return bytes(out[:size])


# ---- the decode rules (lz4_wave_decode's, with the dictionary's match rule) --------------------------------------------------------
class Refused(Exception):
    pass


def decode_block(s, cap, d=b""):
    """the bytes a raw block decodes to at capacity `cap` against dictionary d; raises Refused for CJ_E_CORRUPT"""
    s = bytes(s)
    d = bytes(d)[-WINDOW:]
    n = len(s)
    if cap == 0:
        if n == 1 and s[0] == 0:
            return b""
        raise Refused
    if n == 0:
        raise Refused
    out = bytearray()
    ip = 0
    while True:
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            if ip + 15 >= n:
                raise Refused
            b = s[ip]
            ip += 1; lit += b
            if ip + 15 > n:
                raise Refused
            while b == 255:
                b = s[ip]
                ip += 1; lit += b
                if ip + 15 > n:
                    raise Refused
        rem_out, rem_in = cap - len(out), n - ip
        if rem_out < lit + 12 or rem_in < lit + 8:
            if rem_in != lit or rem_out < lit:
                raise Refused
            out += s[ip:ip + lit]
            return bytes(out)
        out += s[ip:ip + lit]
        ip += lit
        offset = s[ip] | (s[ip + 1] << 8)
        ip += 2
        mlen = token & 15
        if mlen == 15:
            b = s[ip]
            ip += 1; mlen += b
            if ip + 4 > n:
                raise Refused
            while b == 255:
                b = s[ip]
                ip += 1; mlen += b
                if ip + 4 > n:
                    raise Refused
        mlen += 4
        op = len(out)
        if offset == 0 or offset > op + len(d):
            raise Refused
        if cap - op < mlen + 5:
            raise Refused
        if offset > op:
            back = offset - op
            k = min(mlen, back)
            out += d[len(d) - back:len(d) - back + k]
            mlen -= k
        if mlen:
            if offset >= mlen:
                out += out[len(out) - offset:len(out) - offset + mlen]
            else:
                pat = bytes(out[len(out) - offset:])
                out += (pat * (mlen // offset + 1))[:mlen]


def prologue(s, cap, prefix):
    """lz4_block_prologue: (error or 0, stream, capacity)"""
    if prefix:
        if len(s) < 4:
            return NO_PREFIX, s, cap
        size = struct.unpack("<i", s[:4])[0]
        if size < 0:
            return NEG_PREFIX, s, cap
        if size > 0x7E000000:
            return PREFIX_TOO_BIG, s, cap
        if size > cap:
            return OUT_TOO_SMALL, s, cap
        return 0, s[4:], size
    if cap > 0xFFFFFFFF or cap >= 1 << 31:
        return NEG_PREFIX, s, cap
    if cap > 0x7E000000:
        return PREFIX_TOO_BIG, s, cap
    return 0, s, cap


def decode(s, cap, d=b"", prefix=False):
    """(result, bytes) of one chunk of a batch: what cj_dict_batch_* (decompress) give"""
    err, s, cap = prologue(bytes(s), cap, prefix)
    if err:
        return err, b""
    try:
        out = decode_block(s, cap, d)
    except Refused:
        return CORRUPT, b""
    return len(out), out


def size_walk(s, dict_len=0):
    """the size walk (lz4_size_walk.hpp) with a dictionary of dict_len bytes: the decoded size with room that never runs out, or CORRUPT"""
    s = bytes(s)
    n = len(s)
    hist = min(dict_len, WINDOW)
    if n == 0:
        return CORRUPT
    ip = op = 0
    while True:
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            if ip + 15 >= n:
                return CORRUPT
            b = s[ip]
            ip += 1; lit += b
            if ip + 15 > n:
                return CORRUPT
            while b == 255:
                b = s[ip]
                ip += 1; lit += b
                if ip + 15 > n:
                    return CORRUPT
        rem_in = n - ip
        if rem_in < lit + 8:
            if rem_in != lit:
                return CORRUPT
            op += lit
            return PREFIX_TOO_BIG if op > 0x7E000000 else op
        ip += lit
        op += lit
        offset = s[ip] | (s[ip + 1] << 8)
        ip += 2
        mlen = token & 15
        if mlen == 15:
            b = s[ip]
            ip += 1; mlen += b
            if ip + 4 > n:
                return CORRUPT
            while b == 255:
                b = s[ip]
                ip += 1; mlen += b
                if ip + 4 > n:
                    return CORRUPT
        if offset == 0 or offset > op + hist:
            return CORRUPT
        op += mlen + 4


def has_offset0(s, cap, d=b""):
    """True when the decode of s is refused AT a match of offset 0 (the documented deviation (1): liblz4 reads such a match as a run)"""
    s = bytes(s)
    try:
        decode_block(s, cap, d)
        return False
    except Refused:
        pass
    # the same walk, stopping at the first refusal: was it the offset?
    marker = []
    try:
        _decode_trace(s, cap, bytes(d)[-WINDOW:], marker)
    except Refused:
        pass
    return bool(marker)


def _decode_trace(s, cap, d, marker):
    n = len(s)
    if cap == 0 or n == 0:
        raise Refused
    op = ip = 0
    while True:
        token = s[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            if ip + 15 >= n:
                raise Refused
            b = s[ip]
            ip += 1; lit += b
            if ip + 15 > n:
                raise Refused
            while b == 255:
                b = s[ip]
                ip += 1; lit += b
                if ip + 15 > n:
                    raise Refused
        rem_out, rem_in = cap - op, n - ip
        if rem_out < lit + 12 or rem_in < lit + 8:
            raise Refused
        ip += lit; op += lit
        offset = s[ip] | (s[ip + 1] << 8)
        ip += 2
        mlen = token & 15
        if mlen == 15:
            b = s[ip]
            ip += 1; mlen += b
            if ip + 4 > n:
                raise Refused
            while b == 255:
                b = s[ip]
                ip += 1; mlen += b
                if ip + 4 > n:
                    raise Refused
        mlen += 4
        if offset == 0:
            marker.append(ip)
            raise Refused
        if offset > op + len(d) or cap - op < mlen + 5:
            raise Refused
        op += mlen


# ---- hand-written streams --------------------------------------------------------------------------------------------------------
def _ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255); v -= 255
    out.append(v)
    return bytes(out)


def seq(lits, offset, mlen):
    """one sequence: literals, then a match of mlen >= 4 bytes at `offset`"""
    lit, code = len(lits), mlen - 4
    out = bytes([(min(lit, 15) << 4) | min(code, 15)])
    if lit >= 15:
        out += _ext(lit - 15)
    out += lits + struct.pack("<H", offset)
    if code >= 15:
        out += _ext(code - 15)
    return out


def last(lits):
    lit = len(lits)
    return bytes([min(lit, 15) << 4]) + (_ext(lit - 15) if lit >= 15 else b"") + lits


def hand_streams():
    """(name, stream, capacity, dictionary length, accepted) — the edges of the dictionary's match rule and of the end of a block"""
    L = words(400, 77)          # literal material
    T = b"tail!"
    H = []
    add = lambda name, s, cap, dl, ok: H.append((name, s, cap, dl, ok))
    # a first sequence with no literals and a match into the dictionary
    add("first_match_into_dict", seq(b"", 5, 8) + last(T), 13, 7, True)
    add("first_match_into_dict_4096", seq(b"", 4096, 30) + last(T), 35, 4096, True)
    add("first_match_one_byte_dict", seq(b"", 1, 8) + last(T), 13, 1, True)                       # one dictionary byte, then a run of it
    # offset == op + dict_len is the dictionary's first byte; one more is outside
    add("offset_op_plus_dict", seq(L[:3], 10, 8) + last(T), 16, 7, True)
    add("offset_op_plus_dict_plus_1", seq(L[:3], 11, 8) + last(T), 16, 7, False)
    add("offset_op_plus_dict_4096", seq(L[:20], 4116, 9) + last(T), 34, 4096, True)
    add("offset_op_plus_dict_4096_plus_1", seq(L[:20], 4117, 9) + last(T), 34, 4096, False)
    add("offset_65535_from_op_0", seq(b"", 65535, 12) + last(T), 17, 65535, True)
    add("offset_65535_tail_of_70000", seq(L[:1], 65535, 12) + last(T), 18, 70000, True)
    add("offset_65535_dict_65534", seq(b"", 65535, 12) + last(T), 17, 65534, False)
    add("offset_0", seq(L[:4], 0, 8) + last(T), 17, 4096, False)
    # a match that starts in the dictionary and runs into the output with offset < mlen: the remainder is periodic
    add("dict_then_periodic", seq(L[:2], 10, 40) + last(T), 47, 4096, True)
    add("dict_1_then_run", seq(L[:1], 2, 200) + last(T), 206, 4096, True)
    # a dictionary part and a remainder longer than a wavefront is wide
    add("dict_100_rest_200", seq(L[:20], 120, 300) + last(T), 325, 4096, True)
    add("dict_100_rest_65_exact", seq(L[:150], 250, 165) + last(T), 320, 4096, True)               # remainder not periodic (offset > rest)
    add("dict_3000_rest_2000", seq(L[:7], 3007, 5000) + last(T), 5012, 4096, True)                 # both parts above the wide copy's threshold
    add("dict_only_64", seq(L[:5], 505, 64) + last(T), 74, 4096, True)
    add("dict_only_65", seq(L[:5], 505, 65) + last(T), 75, 4096, True)
    add("dict_ends_exactly", seq(L[:5], 69, 64) + last(T), 74, 4096, True)                         # the match is the dictionary's last 64 bytes
    # a chunk above 64 KiB: late matches cannot reach the dictionary any more
    big = seq(L[:70], 1, 70000) + seq(L[70:90], 65535, 20) + last(T)
    add("above_64k_late_match_in_output", big, 70 + 70000 + 20 + 20 + 5, 4096, True)
    add("above_64k_no_dict_needed", big, 70 + 70000 + 20 + 20 + 5, 1, True)
    add("late_offset_past_small_dict", seq(L[:100], 108, 8) + last(T), 113, 7, False)
    add("late_offset_at_small_dict", seq(L[:100], 107, 8) + last(T), 113, 7, True)
    # the end-of-block rules at exact capacity
    add("match_ends_5_before_end", seq(L[:4], 4100, 8) + last(T), 17, 4096, True)
    add("match_ends_4_before_end", seq(L[:4], 4100, 8) + last(T[:4]), 16, 4096, False)
    add("match_one_over_capacity", seq(L[:4], 4100, 9) + last(T), 17, 4096, False)
    add("capacity_one_short", seq(L[:4], 4100, 8) + last(T), 16, 4096, False)
    add("capacity_one_more", seq(L[:4], 4100, 8) + last(T), 18, 4096, True)                        # (decodes to 17: the capacity is only a bound)
    add("literals_only", last(L[:40]), 40, 4096, True)
    add("empty_block", b"\x00", 0, 4096, True)
    add("input_left_over", seq(L[:4], 4100, 8) + last(T) + b"\x00", 17, 4096, False)
    add("match_needs_12_of_room", seq(b"", 5, 4) + last(T), 9, 7, False)                           # fewer than 12 bytes of room: must be the last sequence
    return H


def hand_dict(dict_len):
    return dictionary(dict_len)


# ---- liblz4 (where it loads) ---------------------------------------------------------------------------------------------------
def liblz4():
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    try:
        L = C.CDLL(name)
    except OSError:
        return None
    if not hasattr(L, "LZ4_decompress_safe_usingDict"):
        return None
    L.LZ4_decompress_safe_usingDict.restype = C.c_int
    L.LZ4_decompress_safe_usingDict.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.LZ4_compress_default.restype = C.c_int
    L.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.LZ4_createStream.restype = C.c_void_p
    L.LZ4_freeStream.argtypes = [C.c_void_p]
    L.LZ4_loadDict.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.LZ4_compress_fast_continue.restype = C.c_int
    L.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "LZ4_loadDictHC"):
        L.LZ4_createStreamHC.restype = C.c_void_p
        L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
        L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.LZ4_compress_HC_continue.restype = C.c_int
        L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    return L


def lz4_decode_using_dict(L, s, cap, d):
    """(result, bytes) of LZ4_decompress_safe_usingDict at capacity cap (the dictionary in a buffer of its own, not in front of the output)"""
    out = C.create_string_buffer(max(cap, 1))
    dbuf = C.create_string_buffer(bytes(d), max(len(d), 1))
    r = L.LZ4_decompress_safe_usingDict(bytes(s), out, len(s), cap, dbuf, len(d))
    return r, (out.raw[:r] if r >= 0 else b"")


def lz4_compress_with_dict(L, raw, d, hc=False):
    cap = len(raw) + len(raw) // 255 + 32
    out = C.create_string_buffer(cap)
    dbuf = C.create_string_buffer(bytes(d), max(len(d), 1))
    src = C.create_string_buffer(bytes(raw), max(len(raw), 1))
    if hc:
        st = L.LZ4_createStreamHC()
        L.LZ4_loadDictHC(st, dbuf, len(d))
        r = L.LZ4_compress_HC_continue(st, src, out, len(raw), cap)
        L.LZ4_freeStreamHC(st)
    else:
        st = L.LZ4_createStream()
        L.LZ4_loadDict(st, dbuf, len(d))
        r = L.LZ4_compress_fast_continue(st, src, out, len(raw), cap, 1)
        L.LZ4_freeStream(st)
    assert r > 0
    return out.raw[:r]


def lz4_compress_plain(L, raw):
    cap = len(raw) + len(raw) // 255 + 32
    out = C.create_string_buffer(cap)
    r = L.LZ4_compress_default(bytes(raw), out, len(raw), cap)
    assert r > 0
    return out.raw[:r]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
_cache = {}


def _load():
    if "j" not in _cache:
        with open(os.path.join(GOLDEN, "golden_dict.json")) as f:
            _cache["j"] = json.load(f)
        with open(os.path.join(GOLDEN, "golden_dict.bin"), "rb") as f:
            _cache["b"] = f.read()
    return _cache["j"], _cache["b"]


def valid():
    """the streams liblz4 wrote: name, bytes, n (decoded size), sha256, dict_len, size (the record's class), hc"""
    if "valid" not in _cache:
        j, b = _load()
        _cache["valid"] = [dict(v, bytes=b[v["off"]:v["off"] + v["len"]]) for v in j["valid"]]
    return _cache["valid"]


def mutate(s, pos, val):
    s = bytearray(s)
    s[pos] = val
    return bytes(s)


def mutations():
    """seeded one-byte mutations of valid streams with liblz4's verdict at the original capacity: name, bytes, cap, dict_len, result
    (>= 0 or CORRUPT), sha256"""
    if "mut" not in _cache:
        j, _ = _load()
        vs = valid()
        _cache["mut"] = [dict(m, bytes=mutate(vs[m["base"]]["bytes"], m["pos"], m["val"]), cap=vs[m["base"]]["n"], dict_len=vs[m["base"]]["dict_len"])
                         for m in j["mutations"]]
    return _cache["mut"]


def meta():
    return _load()[0]


def hand():
    """the hand-written streams with what the fixture file records for them: name, bytes, cap, dict_len, result, sha256"""
    j, _ = _load()
    rec = {h["name"]: h for h in j["hand"]}
    return [dict(name=name, bytes=s, cap=cap, dict_len=dl, result=rec[name]["result"], sha256=rec[name]["sha256"], accepted=ok)
            for name, s, cap, dl, ok in hand_streams()]


def cases(dict_len):
    """every fixture stream of one dictionary — valid, mutated, hand-written — as one batch's chunks: name, bytes, cap, result, sha256"""
    out = [dict(name=v["name"], bytes=v["bytes"], cap=v["n"], result=v["n"], sha256=v["sha256"]) for v in valid() if v["dict_len"] == dict_len]
    out += [dict(name=m["name"], bytes=m["bytes"], cap=m["cap"], result=m["result"], sha256=m["sha256"]) for m in mutations() if m["dict_len"] == dict_len]
    out += [dict(name=h["name"], bytes=h["bytes"], cap=h["cap"], result=h["result"], sha256=h["sha256"]) for h in hand() if h["dict_len"] == dict_len]
    return out
