"""The Zstandard encoder's test inputs, seeded: the smallest inputs at which each part of it can go wrong, with the
scalar model (tests/hostsim/zstd_enc_model.c) and the host build of the kernel's entropy stage (tests/hostsim/sim_zstd_encode.cpp)
behind ctypes.  Data and helpers only; nothing here needs a GPU or libzstd."""
import ctypes as C
import os
import subprocess

import deflate_cases as D
from hostsim_build import build_sim

ROOT = D.ROOT
SIM = os.path.join(ROOT, "tests", "hostsim")
OUT_TOO_SMALL, BAD_ARG, INPUT_TOO_LARGE = -6, -101, -1
RAW, RLE, COMPRESSED = 0, 1, 2                   # block types; the literal modes are RAW, RLE, HUF
HUF = 2
PREDEFINED, RLE_MODE, FSE_MODE = 0, 1, 2         # sequence table modes
DIRECT, FSE_WEIGHTS = 1, 2                       # tree description kinds
PIECE = 65536
FLAGS = (0, 1)
SIM_BOUNDS = -9999                               # tests/hostsim/sim_wave.hpp: an access outside the registered ranges
ZINFO, SIM_INFO = 12, 10                         # words a piece of the model's / the host build's report
_cache = {}

# first values of the match-length codes 32 .. 51 and of the literal-length codes 16 .. 34 (RFC 8878 3.1.1.3.2.1.1)
ML_BASES = (35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771)
LL_BASES = (16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
# distances on both sides of every offset code's first value (Offset_Value = distance + 3 = 2^k) that a piece can hold: a match starts
# at most 8 bytes before the piece's end, so no distance above 65 528 — and so neither 65 533 nor 65 535, nor offset code 16 — occurs
DISTANCES = tuple(sorted({d for k in range(2, 16) for d in ((1 << k) - 4, (1 << k) - 3) if d >= 1} | {65000}))


def lib():
    """the model and the host build in one library (built by __graft_entry__.build() or here)"""
    if "lib" not in _cache:
        so = os.path.join(SIM, "libsim_zstd_encode.so")
        srcs = [os.path.join(SIM, f) for f in ("sim_zstd_encode.cpp", "sim_wave.hpp", "zstd_enc_model.c", "enc2_round.h", "deflate_enc_model.c")]
        srcs += [os.path.join(ROOT, "cramjam_amd", "csrc", f) for f in ("zstd_enc_wave.hpp", "zstd_fse_enc.h", "deflate_enc_wave.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            build_lib(so)
        L = C.CDLL(so)
        L.zse_model_compress.restype = C.c_int64
        L.zse_model_compress.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.zse_model_bound.restype = C.c_uint64
        L.zse_model_bound.argtypes = [C.c_uint64, C.c_uint32]
        L.zse_model_records.restype = C.c_uint32
        L.zse_model_records.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.zse_model_xxh64.restype = C.c_uint64
        L.zse_model_xxh64.argtypes = [C.c_void_p, C.c_uint64]
        L.sim_zstd_encode.restype = C.c_longlong
        L.sim_zstd_encode.argtypes = [C.c_uint, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.c_void_p]
        L.sim_zse_table.restype = C.c_longlong
        L.sim_zse_table.argtypes = [C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sim_zsf_table.restype = C.c_longlong
        L.sim_zsf_table.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint] + [C.c_void_p] * 6
        L.sim_zsf_weights.restype = C.c_uint
        L.sim_zsf_weights.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
        L.sim_zse_bound.restype = C.c_ulonglong
        L.sim_zse_bound.argtypes = [C.c_ulonglong, C.c_uint]
        _cache["lib"] = L
    return _cache["lib"]


def build_lib(so=None, extra=()):
    so = so or os.path.join(SIM, "libsim_zstd_encode.so")
    objs = []
    for src in ("zstd_enc_model.c", "deflate_enc_model.c"):      # (both include enc2_round.h: the matcher's round)
        objs.append(so + "." + src + ".o")
        subprocess.check_call(["gcc", "-O2", "-g", "-fPIC", "-Wall", "-Wno-unused-function", "-c", "-o", objs[-1], os.path.join(SIM, src)] + list(extra))
    build_sim(["sim_zstd_encode.cpp"] + objs, so, extra=extra)
    for o in objs:
        os.remove(o)
    return so


def bound(n, flags=0):
    return int(lib().zse_model_bound(n, flags))


def pieces(n):
    return max(1, -(-n // PIECE))


def model(data, flags=0, cap=None):
    """(result, frame, report): report[p] = the ZINFO words of piece p — 0 literal mode, 1 streams, 2 tree kind (1 direct weights, 2 FSE-compressed weights),
    3 / 4 / 5 LL / OF / ML mode, 6 sequences, 7 literals, 8 bits in the sequence stream's last byte before the final bit, 9 block type,
    10 depth of the literals' unlimited Huffman tree, 11 distinct literal bytes"""
    L = lib()
    data = bytes(data)
    b = bound(len(data), flags)
    out = (C.c_ubyte * (b + 8))()
    rep = (C.c_uint32 * (ZINFO * pieces(len(data))))()
    r = L.zse_model_compress(data, len(data), flags, out, b if cap is None else cap, rep)
    return r, bytes(out[:max(r, 0)]), [tuple(rep[ZINFO * p:ZINFO * (p + 1)]) for p in range(pieces(len(data)))]


def records(piece):
    """the matcher's records of one piece: (literal start, literal count, distance, match length)"""
    piece = bytes(piece)
    rec = (C.c_uint32 * (4 * (len(piece) // 4 + 2)))()
    n = lib().zse_model_records(piece, len(piece), rec)
    return [tuple(rec[4 * i:4 * i + 4]) for i in range(n)]


def sim(data, flags, cap, in_mis=0, out_mis=0, guard=64):
    """(result, frame, report) of the host build: the input in_mis, the output out_mis bytes behind a 16-byte boundary, `guard` bytes of
    0xA5 behind the capacity that must stay.  report[p]: the first SIM_INFO words of the model's"""
    L = lib()
    data = bytes(data)
    ibuf = (C.c_ubyte * (len(data) + 32))()
    iat = C.addressof(ibuf) + (-C.addressof(ibuf)) % 16 + in_mis
    C.memmove(iat, data, len(data))
    obuf = (C.c_ubyte * (cap + guard + 32))()
    C.memset(obuf, 0xA5, len(obuf))
    o0 = (-C.addressof(obuf)) % 16 + out_mis
    rep = (C.c_uint32 * (SIM_INFO * pieces(len(data))))()
    r = L.sim_zstd_encode(flags, iat, len(data), C.addressof(obuf) + o0, cap, rep)
    assert r != SIM_BOUNDS, "a stand-in's bounds check fired"
    assert bytes(obuf[o0 + cap:o0 + cap + guard]) == b"\xa5" * guard and bytes(obuf[:o0]) == b"\xa5" * o0, "a store outside the capacity"
    return r, bytes(obuf[o0:o0 + max(r, 0)]), [tuple(rep[SIM_INFO * p:SIM_INFO * (p + 1)]) for p in range(pieces(len(data)))]


def corpus_files():
    import deflate_enc_cases as E
    return E.corpus_files()


def corpus_chunks(path):
    import deflate_enc_cases as E
    return E.corpus_chunks(path)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def rand7(n, seed):
    """n seeded bytes below 128 (a tree of direct weights can describe them), none of them 0"""
    return bytes(1 + b % 127 for b in D.random_bytes(n, seed))


def _search(name, candidates, accept):
    """the first candidate the model's own records or report accept (seeded, bounded)"""
    for c in candidates:
        if accept(c):
            return c
    raise AssertionError("no candidate gives " + name)


def match_length_case(L):
    """600 random bytes A, then A over and over for L bytes (a match at distance 600 that overlaps itself), a byte that differs, a tail"""
    A = D.random_bytes(600, 1000 + L % 997)
    body = (A * (L // 600 + 2))[:L + 1]
    return A + body[:L] + bytes([body[L] ^ 0x5A]) + D.random_bytes(24, 2000 + L % 997)


def literal_length_case(L):
    """a first sequence (700 bytes Z, Z's head again), then exactly L fresh literals, then 40 bytes from inside Z: a sequence whose literal
    length is L"""
    def make(seed):
        Z = D.random_bytes(700, 3000 + seed)
        return Z + Z[:32] + bytes(b ^ 0xFF for b in D.random_bytes(L, 3100 + seed)) + Z[100:140] + D.random_bytes(24, 3200 + seed)
    return _search("literal length %d" % L, (make(L % 89 + 100 * k) for k in range(40)), lambda d: any(r[1] == L and r[3] for r in records(d)))


def distance_case(d):
    import deflate_enc_cases as E
    leads = range(600, 800) if d < 60000 else range(8, 208)
    return _search("distance %d" % d, (E.distance_case(d, lead) for lead in leads), lambda c: len(c) <= PIECE and any(r[2] == d and r[3] >= 4 for r in records(c)))


def literal_count_case(T):
    """a piece of exactly T literals in a Compressed block: random bytes below 128, which become literals, then text whose length is searched"""
    head = rand7(max(T - 200, 0), 4000 + T) if T > 300 else b""

    def ok(c):
        rep = model(c)[2][0]
        return rep[9] == COMPRESSED and rep[7] == T
    if T <= 64:
        return _few_literals(T)
    return _search("%d literals" % T, (head + D.words(n, 4300 + T) for n in range(60, 6000, 1)), ok)


def _few_literals(T):
    """T distinct literals and nothing else: T fresh bytes, then those bytes again and again (one long match)"""
    def ok(c):
        rep = model(c)[2][0]
        return rep[9] == COMPRESSED and rep[7] == T
    return _search("%d literals" % T, (bytes(range(40, 40 + T)) * k for k in range(6, 40)), ok)


def sequence_count_case(N):
    """exactly N sequences: N markers of 16 bytes behind 2048 random bytes that hold them"""
    def make(k, seed):
        Z = D.random_bytes(2048, 5000 + seed)
        out = bytearray(Z)
        for j in range(k):
            out += Z[16 * j:16 * j + 16] + bytes([j & 0xFF, 0xA5 ^ j & 0xFF, seed & 0xFF])
        return bytes(out) + D.random_bytes(24, 5100 + seed)
    return _search("%d sequences" % N, (make(k, s) for s in range(4) for k in range(max(N - 6, 1), min(N + 8, 128) + 1)), lambda c: model(c)[2][0][6] == N and model(c)[2][0][9] == COMPRESSED)


def no_match_piece(n, skew):
    """n bytes without a repeat of four: the odd bytes run through every pair of 100 values once, the even bytes take few values (100 + k)
    with the counts skew[k]; every byte is below 128"""
    fill = []
    for a in range(100):
        fill.append(a)
        for b in range(a + 1, 100):
            fill += [a, b]
    pool = bytearray()
    for k, c in enumerate(skew):
        pool += bytes([100 + k]) * c
    assert len(pool) >= n // 2 and len(fill) >= n // 2
    pool = pool[:n // 2]
    g = D._lcg(99)
    for i in range(len(pool) - 1, 0, -1):
        j = next(g) % (i + 1)
        pool[i], pool[j] = pool[j], pool[i]
    out = bytearray(n)
    out[0::2], out[1::2] = pool, bytes(fill[:n // 2])
    return bytes(out)


def fibonacci_piece():
    fib = [1, 2]
    while sum(fib) + fib[-1] + fib[-2] <= 8000:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += 8000 - sum(fib)
    return no_match_piece(16000, fib)


def equal128_piece(first=1):
    """64 seeded permutations of 128 byte values from `first` on.  From 1: 128 listed weights, 0 and 1 (FSE-compressed); from 0: 127
    listed weights that are all 1, which an FSE description cannot say (one distinct symbol): direct weights"""
    g = D._lcg(77)
    out = bytearray()
    for _ in range(64):
        p = list(range(first, first + 128))
        for i in range(127, 0, -1):
            j = next(g) % (i + 1)
            p[i], p[j] = p[j], p[i]
        out += bytes(p)
    return bytes(out)


def skewed256_piece():
    g = D._lcg(78)
    return bytes(range(256)) + bytes(min(next(g) % 256, next(g) % 256, next(g) % 256) for _ in range(12000))


def two_symbol_piece():
    """literals of two values only, enough of them for a tree to pay: bits of a seeded generator as bytes, cut where the model codes them"""
    g = D._lcg(79)
    bits = bytes(0x61 + ((next(g) >> 7) & 1) for _ in range(20000))
    return _search("two-symbol Huffman literals", (bits[:n] for n in range(600, 20000, 200)), lambda c: model(c)[2][0][0] == HUF and model(c)[2][0][11] == 2)


def predefined_piece():
    """a short piece where the predefined distributions win for all three tables: a description would cost more than it saves"""
    return _search("a piece of three Predefined tables", (D.words(n, 7000 + n) for n in range(150, 1500, 7)),
                   lambda c: model(c)[2][0][9] == COMPRESSED and model(c)[2][0][6] >= 8 and model(c)[2][0][3:6] == (PREDEFINED,) * 3)


def fse_piece():
    """a long one where FSE_Compressed wins for all three"""
    return _search("a piece of three FSE_Compressed tables", (D.words(n, 7100 + n) for n in range(3000, 30000, 1000)),
                   lambda c: model(c)[2][0][3:6] == (FSE_MODE,) * 3)


def repeat_cases():
    """name -> data: the repeat code's situations — two matches at one distance with literals between, the frame's first sequence at
    distance 1, the pair split across two pieces — and one long match of period 2 that overlaps itself (tests/test_zstd_encode_model.py
    asserts each from the records)"""
    Z, X = D.random_bytes(700, 6000), D.random_bytes(64, 6001)
    between = Z + Z[:40] + X[:5] + Z[45:85] + X[8:40]
    first1 = X[:10] + b"a" * 400 + X[10:40]
    tail1 = D.random_bytes(PIECE - 700 - 40 - 40, 6002) + Z + Z[:40] + X[:40]
    Z2 = D.random_bytes(700, 6003)
    split = tail1 + Z2 + Z2[:40] + X[:40]
    return {"rep_between": between, "period2": b"ab" * 3000 + X[:24], "rep_first": first1, "rep_split": split}


def bit_offset_texts():
    """short texts whose sequence stream ends at each of the 8 bit offsets before the final bit: offset -> text"""
    if "bits" not in _cache:
        found = {}
        for seed in range(600):
            t = D.words(120 + seed % 200, 8000 + seed)
            rep = model(t)[2][0]
            if rep[9] == COMPRESSED and rep[6]:
                found.setdefault(rep[8], t)
            if len(found) == 8:
                break
        _cache["bits"] = found
    return _cache["bits"]


def three_pieces():
    return D.words(PIECE, 21) + D.random_bytes(PIECE, 22) + D.words(3000, 23)


def cases():
    """name -> data, every case of DESIGN.md 5.15's list"""
    if "cases" not in _cache:
        cs = {}
        for n in range(66):
            cs["len%d" % n] = D.words(n, 100 + n)
        for n in (5, 40, 65536, 65537, 131073):
            cs["one%d" % n] = b"a" * n
        for n in (255, 256, 65535, 65536, 65537, 65791, 65792):
            cs["random%d" % n] = D.random_bytes(n, 3)
        cs["text_random_text"] = three_pieces()
        for T in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384):
            cs["lits%d" % T] = literal_count_case(T)
        cs["seq0"] = no_match_piece(6000, [3000, 600, 300, 200])
        for N in (1, 127, 128):
            cs["seq%d" % N] = sequence_count_case(N)
        for d in DISTANCES:
            cs["dist%d" % d] = distance_case(d)
        for b in ML_BASES:
            cs["mlen%d" % (b - 1)], cs["mlen%d" % b] = match_length_case(b - 1), match_length_case(b)
        for b in LL_BASES:
            cs["llen%d" % (b - 1)], cs["llen%d" % b] = literal_length_case(b - 1), literal_length_case(b)
        cs.update(repeat_cases())
        cs["huf_two"], cs["huf_equal128"], cs["huf_skewed256"], cs["huf_fibonacci"] = two_symbol_piece(), equal128_piece(), skewed256_piece(), fibonacci_piece()
        cs["huf_direct127"] = equal128_piece(0)
        cs["text4k"], cs["text100"] = D.words(4096, 2), D.words(100, 1)
        cs["fse_predefined"], cs["fse_all"] = predefined_piece(), fse_piece()
        Z = D.random_bytes(700, 6100)
        cs["fse_rle"] = Z + b"".join(Z[50 * k:50 * k + 40] + bytes([k, 255 - k, 7, k ^ 0x55, 9]) for k in range(6)) + D.random_bytes(24, 6101)
        for off, t in sorted(bit_offset_texts().items()):
            cs["endbit%d" % off] = t
        _cache["cases"] = cs
    return _cache["cases"]


def coverage():
    """what the cases reach, from the model's own report: sets of block types, literal modes, stream counts, header forms (bytes of a
    literals header by mode), sequence-count forms and the three tables' modes"""
    if "cov" not in _cache:
        cov = {"block": set(), "lit": set(), "streams": set(), "tree": set(), "lit_header": set(), "nseq_form": set(), "ll": set(), "of": set(), "ml": set(), "head": set()}
        for name, data in cases().items():
            cov["head"].add(6 if len(data) <= 255 else 7 if len(data) <= 65536 else 8 if len(data) <= 65791 else 10)
            for rep in model(data)[2]:
                cov["block"].add(rep[9])
                if rep[9] != COMPRESSED:
                    continue
                cov["lit"].add(rep[0]); cov["nseq_form"].add(0 if rep[6] == 0 else 1 if rep[6] < 128 else 2)
                n = rep[7]
                cov["lit_header"].add((rep[0], (3 if n <= 1023 else 4 if n <= 16383 else 5) if rep[0] == HUF else (1 if n <= 31 else 2 if n <= 4095 else 3)))
                if rep[0] == HUF:
                    cov["streams"].add(rep[1]); cov["tree"].add(rep[2])
                if rep[6]:
                    cov["ll"].add(rep[3]); cov["of"].add(rep[4]); cov["ml"].add(rep[5])
        _cache["cov"] = cov
    return _cache["cov"]


def write_cases_file(path):
    """the file a stand-alone build of tests/hostsim/sim_zstd_encode.cpp (-DSIM_MAIN) runs: every case x flag at capacities the bound,
    exact, exact - 1 and 0, the alignments in turn, with the model's verdict and bytes.  Format: u32 count, then per case u32 flags, n, cap,
    input misalignment, output misalignment | i64 expected result | the input | the expected frame (result > 0).  Returns the count.
    (Both models include the matcher's round, tests/hostsim/enc2_round.h, from their own directory.)
        python -c "import sys; sys.path.insert(0, 'tests'); import zstd_enc_cases as E; print(E.write_cases_file('cases.bin'))"
        gcc -O1 -g -fsanitize=address,undefined -c -o zmodel.o tests/hostsim/zstd_enc_model.c
        gcc -O1 -g -fsanitize=address,undefined -c -o dmodel.o tests/hostsim/deflate_enc_model.c
        python -c "import os, sys; sys.path.insert(0, 'tests'); from hostsim_build import build_sim; build_sim(['sim_zstd_encode.cpp', os.path.abspath('zmodel.o'), os.path.abspath('dmodel.o')], 'sim_main', main=True, sanitize=True)" && ./sim_main cases.bin"""
    import struct
    rows = []
    for k, (name, data) in enumerate(cases().items()):
        for flags in FLAGS:
            r, s, _ = model(data, flags)
            for j, cap in enumerate((bound(len(data), flags), r, r - 1, 0)):
                verdict = r if cap >= r else OUT_TOO_SMALL
                mi, mo = ((0, 0), (1, 5), (3, 15))[(k + j) % 3]
                rows.append(struct.pack("<5Iq", flags, len(data), cap, mi, mo, verdict) + data + (s if verdict > 0 else b""))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(rows)) + b"".join(rows))
    return len(rows)
