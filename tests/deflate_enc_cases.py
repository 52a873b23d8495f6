"""The DEFLATE encoder's test inputs, seeded: the smallest inputs at which each part of it can go wrong, with the
scalar model (tests/hostsim/deflate_enc_model.c) and the host build of the kernel's entropy stage (tests/hostsim/sim_deflate_encode.cpp)
behind ctypes.  Data and helpers only; nothing here needs a GPU."""
import bz2
import ctypes as C
import glob
import os
import subprocess

import deflate_cases as D
from hostsim_build import build_sim

ROOT = D.ROOT
SIM = os.path.join(ROOT, "tests", "hostsim")
RAW, ZLIB, GZIP, WRAPS, WBITS, WRAP_NAME = D.RAW, D.ZLIB, D.GZIP, D.WRAPS, D.WBITS, D.WRAP_NAME
OUT_TOO_SMALL, BAD_ARG, INPUT_TOO_LARGE = -6, -101, -1
STORED, FIXED, DYNAMIC = 0, 1, 2
PIECE = 65536
_cache = {}

MATCH_LENGTHS = (4, 5, 10, 11, 18, 19) + tuple(range(257, 263)) + tuple(range(515, 521))
_BASES = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DISTANCES = tuple(sorted({1} | {b - 1 for b in _BASES if b > 1} | set(_BASES) | {32767, 32768}))      # both sides of every distance code's first value
TOO_FAR = (32769, 33000, 36000, 40000)
SIM_BOUNDS = -9999                               # tests/hostsim/sim_wave.hpp: an access outside the registered ranges


def lib():
    """the model and the host build in one library (built by __graft_entry__.build() or here)"""
    if "lib" not in _cache:
        so = os.path.join(SIM, "libsim_deflate_encode.so")
        srcs = [os.path.join(SIM, "sim_deflate_encode.cpp"), os.path.join(SIM, "sim_wave.hpp"), os.path.join(SIM, "deflate_enc_model.c"), os.path.join(SIM, "enc2_round.h"), os.path.join(ROOT, "cramjam_amd", "csrc", "deflate_enc_wave.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            build_lib(so)
        L = C.CDLL(so)
        L.dfe_model_compress.restype = C.c_int64
        L.dfe_model_compress.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.dfe_model_bound.restype = C.c_uint64
        L.dfe_model_bound.argtypes = [C.c_uint64, C.c_int]
        L.dfe_model_records.restype = C.c_uint32
        L.dfe_model_records.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.dfe_model_build_lens.restype = C.c_uint32
        L.dfe_model_build_lens.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.sim_deflate_encode.restype = C.c_longlong
        L.sim_deflate_encode.argtypes = [C.c_int, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_void_p]
        L.sim_dfe_build_lens.restype = C.c_longlong
        L.sim_dfe_build_lens.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_void_p]
        L.sim_dfe_assign_codes.restype = C.c_longlong
        L.sim_dfe_assign_codes.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
        L.sim_dfe_bound.restype = C.c_ulonglong
        L.sim_dfe_bound.argtypes = [C.c_ulonglong, C.c_int]
        _cache["lib"] = L
    return _cache["lib"]


def build_lib(so=None, extra=()):
    so = so or os.path.join(SIM, "libsim_deflate_encode.so")
    obj = so + ".model.o"
    subprocess.check_call(["gcc", "-O2", "-g", "-fPIC", "-Wall", "-c", "-o", obj, os.path.join(SIM, "deflate_enc_model.c")] + list(extra))
    build_sim(["sim_deflate_encode.cpp", obj], so, extra=extra)
    os.remove(obj)
    return so


def bound(n, wrap):
    return int(lib().dfe_model_bound(n, wrap))


def model(data, wrap, cap=None):
    """(result, stream, block types, [deepest unlimited literal/length tree, distance tree, bits in the last byte])"""
    L = lib()
    data = bytes(data)
    b = bound(len(data), wrap)
    out = (C.c_ubyte * (b + 8))()
    types = (C.c_ubyte * (len(data) // PIECE + 2))()
    info = (C.c_uint32 * 3)()
    r = L.dfe_model_compress(data, len(data), wrap, out, b if cap is None else cap, types, info)
    return r, bytes(out[:max(r, 0)]), list(types[:max(1, -(-len(data) // PIECE))]), list(info)


def records(piece):
    """the matcher's records of one piece: (literal start, literal count, distance, match length)"""
    piece = bytes(piece)
    rec = (C.c_uint32 * (4 * (len(piece) // 4 + 2)))()
    n = lib().dfe_model_records(piece, len(piece), rec)
    return [tuple(rec[4 * i:4 * i + 4]) for i in range(n)]


def sim(data, wrap, cap, in_mis=0, out_mis=0, guard=64):
    """(result, stream) of the host build: the input in_mis, the output out_mis bytes behind a 16-byte boundary, `guard` bytes of 0xA5
    behind the capacity that must stay"""
    L = lib()
    data = bytes(data)
    ibuf = (C.c_ubyte * (len(data) + 32))()
    iat = C.addressof(ibuf) + (-C.addressof(ibuf)) % 16 + in_mis
    C.memmove(iat, data, len(data))
    obuf = (C.c_ubyte * (cap + guard + 32))()
    C.memset(obuf, 0xA5, len(obuf))
    o0 = (-C.addressof(obuf)) % 16 + out_mis
    r = L.sim_deflate_encode(wrap, iat, len(data), C.addressof(obuf) + o0, cap, None)
    assert r != SIM_BOUNDS, "a stand-in's bounds check fired"
    assert bytes(obuf[o0 + cap:o0 + cap + guard]) == b"\xa5" * guard and bytes(obuf[:o0]) == b"\xa5" * o0, "a store outside the capacity"
    return r, bytes(obuf[o0:o0 + max(r, 0)])


def corpus_files():
    return sorted(glob.glob(os.path.join(D.GOLDEN, "corpus", "*.bz2")))


def corpus_chunks(path):
    with open(path, "rb") as f:
        d = bz2.decompress(f.read())
    return [d[i:i + PIECE] for i in range(0, len(d), PIECE)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def match_length_case(L):
    """600 random bytes A, A[:L], a byte that differs, a random tail (the matcher starts no match in the last 8 bytes)"""
    A = D.random_bytes(600, 1000 + L)
    return A + A[:L] + bytes([A[L] ^ 0x5A]) + D.random_bytes(24, 2000 + L)


def distance_case(d, lead=600):
    """a 16-byte marker and its repeat d bytes on (d < 16: the marker runs into itself), zeros in between so that the table keeps the
    marker; nothing around them matches"""
    pre = D.random_bytes(lead, 3000 + d)[:-1] + b"\x01"
    M = bytes(1 + b % 255 for b in D.random_bytes(16, 4000 + d))
    body = bytearray(M[:d] if d < 16 else M + bytes(d - 16))
    for _ in range(16):
        body.append(body[-d])
    return pre + bytes(body) + bytes(1 + b % 255 for b in D.random_bytes(24, 5000 + d))


def distance_cases():
    """name -> (distance, data): the lead is searched (seeded, at most 200 tries) until the model's records hold a match at that
    distance — a position sees the table as it was before its own block of 128, so a short distance is found only across a block edge"""
    if "dist" not in _cache:
        out = {}
        for d in DISTANCES:
            for lead in range(600, 800):
                data = distance_case(d, lead)
                if any(r[2] == d and r[3] >= 4 for r in records(data)):
                    out["dist%d" % d] = (d, data)
                    break
            else:
                raise AssertionError("no lead gives a match at distance %d" % d)
        for d in TOO_FAR:
            out["far%d" % d] = (d, distance_case(d))
        _cache["dist"] = out
    return _cache["dist"]


def fibonacci_piece():
    """64 KiB whose even bytes take 21 values with the Fibonacci counts 1, 2, 3, 5, ... (the end-of-block symbol is the sequence's other
    1; the most frequent value takes what is left of the 32 768), in a seeded order, and whose odd bytes run through 200 other values
    so that no pair of them comes twice (a de Bruijn sequence of order 2): no four bytes repeat, the matcher finds nothing, and the
    rare values hang in one chain"""
    fill = []
    for a in range(200):
        fill.append(a)
        for b in range(a + 1, 200):
            fill += [a, b]
    fib = [1, 2]
    while sum(fib) + fib[-1] + fib[-2] <= PIECE // 2:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += PIECE // 2 - sum(fib)
    pool = bytearray()
    for k, c in enumerate(fib):
        pool += bytes([200 + k]) * c
    g = D._lcg(99)
    for i in range(len(pool) - 1, 0, -1):           # seeded shuffle
        j = next(g) % (i + 1)
        pool[i], pool[j] = pool[j], pool[i]
    out = bytearray(PIECE)
    out[0::2], out[1::2] = pool, bytes(fill[:PIECE // 2])
    return bytes(out)


def deep_corpus_chunks():
    """the chunks of paper-100k and ooffice whose unlimited literal/length tree is deeper than 15: (name, chunk)"""
    if "deep" not in _cache:
        out = []
        for f in corpus_files():
            base = os.path.basename(f)
            if base.startswith(("paper-100k", "ooffice")):
                for k, c in enumerate(corpus_chunks(f)):
                    if model(c, RAW)[3][0] > 15:
                        out.append(("%s_%d" % (base.split(".")[0], k), c))
        _cache["deep"] = out
    return _cache["deep"]


def fixed_text():
    """a 300-byte text whose fixed-code cost is below the dynamic one: a sentence of 50 bytes six times over — few symbols, so the
    dynamic header outweighs what its codes save (the first seed that gives it)"""
    if "fixed" not in _cache:
        for seed in range(200):
            t = (D.words(50, 7000 + seed) * 6)[:300]
            if model(t, RAW)[2] == [FIXED]:
                _cache["fixed"] = t
                break
        else:
            raise AssertionError("no seed gives a fixed block")
    return _cache["fixed"]


def bit_offset_texts():
    """short texts whose last block ends at each of the 8 bit offsets: offset -> text"""
    if "bits" not in _cache:
        found = {}
        for seed in range(400):
            t = D.words(20 + seed % 50, 8000 + seed)
            found.setdefault(model(t, RAW)[3][2], t)
            if len(found) == 8:
                break
        _cache["bits"] = found
    return _cache["bits"]


def three_pieces():
    return D.words(PIECE, 21) + D.random_bytes(PIECE, 22) + D.words(3000, 23)


def cases():
    """name -> data, every case of DESIGN.md 5.13's list"""
    if "cases" not in _cache:
        cs = {}
        for n in (0, 1, 2, 3, 7, 8, 12, 13, 64, 65):
            cs["len%d" % n] = D.words(n, 100 + n)
        cs["one5"], cs["one40"], cs["zeros64k"] = b"a" * 5, b"a" * 40, bytes(PIECE)
        for L in MATCH_LENGTHS:
            cs["mlen%d" % L] = match_length_case(L)
        for name, (_, data) in distance_cases().items():
            cs[name] = data
        cs["fibonacci"] = fibonacci_piece()
        for name, c in deep_corpus_chunks()[:2]:
            cs["deep_" + name] = c
        for n in (65535, 65536, 65537):
            cs["random%d" % n] = D.random_bytes(n, 3)
        cs["text_random_text"] = three_pieces()
        cs["fixed300"] = fixed_text()
        for off, t in sorted(bit_offset_texts().items()):
            cs["endbit%d" % off] = t
        cs["text4k"] = D.words(4096, 2)
        _cache["cases"] = cs
    return _cache["cases"]


def write_cases_file(path):
    """the file a stand-alone build of tests/hostsim/sim_deflate_encode.cpp (-DSIM_MAIN) runs: every case x wrapper at capacities the bound,
    exact, exact - 1 and 0, the alignments in turn, with the model's verdict and bytes.  Format: u32 count, then per case u32 wrap, n, cap,
    input misalignment, output misalignment | i64 expected result | the input | the expected stream (result > 0).  Returns the count.
    (The model includes the matcher's round, tests/hostsim/enc2_round.h, from its own directory.)
        python -c "import sys; sys.path.insert(0, 'tests'); import deflate_enc_cases as E; print(E.write_cases_file('cases.bin'))"
        gcc -O1 -g -fsanitize=address,undefined -c -o model.o tests/hostsim/deflate_enc_model.c
        python -c "import os, sys; sys.path.insert(0, 'tests'); from hostsim_build import build_sim; build_sim(['sim_deflate_encode.cpp', os.path.abspath('model.o')], 'sim_main', main=True, sanitize=True)" && ./sim_main cases.bin"""
    import struct
    rows = []
    for k, (name, data) in enumerate(cases().items()):
        for wrap in WRAPS:
            r, s, _, _ = model(data, wrap)
            for j, cap in enumerate((bound(len(data), wrap), r, r - 1, 0)):
                verdict = r if cap >= r else OUT_TOO_SMALL
                mi, mo = ((0, 0), (1, 5), (3, 15))[(k + j) % 3]
                rows.append(struct.pack("<5Iq", wrap, len(data), cap, mi, mo, verdict) + data + (s if verdict > 0 else b""))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(rows)) + b"".join(rows))
    return len(rows)
