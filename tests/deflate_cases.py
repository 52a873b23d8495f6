"""DEFLATE test material shared by tests/test_deflate_model.py, tests/test_deflate_gpu.py and tests/golden/make_golden_deflate.py:
the payloads and their matrix, the hand-written streams (a bit writer, no compressor), zlib's verdict at a capacity computed live
(Python's zlib module), the size query's expectation derived from it, the loaders of tests/golden/golden_deflate.json + .bin and of
golden_deflate_others.json + .bin (libdeflate's and zopfli's streams) and the host build of the kernel's decoder (tests/hostsim/sim_deflate_decode.cpp).  Data and helpers only; nothing here needs a GPU."""
import bz2
import ctypes as C
import hashlib
import json
import os
import zlib

from hostsim_build import SIM_DIR, build_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

RAW, ZLIB, GZIP = 0, 1, 2                         # cj_deflate_wrap
WRAPS = (RAW, ZLIB, GZIP)
WRAP_NAME = {RAW: "raw", ZLIB: "zlib", GZIP: "gzip"}
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
OUT_TOO_SMALL, BAD_ARG = -6, -101
CORRUPT, HEADER, CHECKSUM, EOF, TRAILING = -40, -41, -42, -43, -44
LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)
STRATEGY_NAME = {zlib.Z_DEFAULT_STRATEGY: "default", zlib.Z_FIXED: "fixed", zlib.Z_HUFFMAN_ONLY: "huff", zlib.Z_RLE: "rle"}

# Fixture IDs whose verdict differs from zlib's ON PURPOSE, with the reason (at most 2 % of the fixtures; tests assert that).  None:
# the decoder takes every accept / reject decision where inflate takes it.
DIVERGES_FROM_ZLIB = {}


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- payloads -----------------------------------------------------------------------------------------------------------------------
def _lcg(seed):
    x = (seed * 2654435761 + 12345) & 0xFFFFFFFF
    while True:
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        yield x >> 8


def words(n, seed):
    """n bytes of word-like text from a vocabulary of 400 words (a generator of our own: the same bytes everywhere)"""
    g = _lcg(seed)
    vocab = []
    for _ in range(400):
        ln = 2 + next(g) % 8
        vocab.append(bytes(97 + next(g) % 26 for _ in range(ln)))
    out = bytearray()
    while len(out) < n:
        out += vocab[next(g) % 400 if next(g) % 4 else next(g) % 20]
        out += b" " if next(g) % 9 else b".\n"
    return bytes(out[:n])


def random_bytes(n, seed):
    g = _lcg(seed)
    return bytes(next(g) & 0xFF for _ in range(n))


def corpus_chunk():
    with open(os.path.join(GOLDEN, "corpus", "alice29.txt.bz2"), "rb") as f:
        return bz2.decompress(f.read())[:65536]


def payloads():
    """name -> bytes, in the order of the issue's list (the 300 000-byte text is flush_text, written apart).  dist32768 repeats at
    distance 32 768, but zlib's own streams of it stop at distance 32 506 (w_size - MIN_LOOKAHEAD): distances 32 767 and 32 768 are
    written by tests/deflate_synth.py (family `matches`) and by the other encoders of tests/golden/golden_deflate_others.*"""
    half = words(32768, 11)
    return {"empty": b"", "one": b"Q", "text300": words(300, 1), "text4k": words(4096, 2), "corpus64k": corpus_chunk(), "zeros64k": bytes(65536),
            "random64k": random_bytes(65536, 3), "dist32768": half + half}


# The small payloads get the full cross of level x strategy x wrapper; the 64 KiB ones the combinations listed here (level 0 and random
# bytes are 64 KiB a stream), so that each fixture file stays under 1 MiB: every level, strategy and wrapper still meets a 64 KiB payload
_D, _F, _H, _R = STRATEGIES
THINNED = {
    "corpus64k": ((1, _D, RAW), (6, _D, ZLIB), (9, _D, GZIP), (6, _F, RAW), (6, _H, GZIP), (6, _R, ZLIB)),
    "zeros64k": ((0, _D, RAW),) + tuple((lv, st, w) for lv in (1, 6, 9) for st in STRATEGIES for w in WRAPS),
    "random64k": ((0, _D, GZIP), (6, _D, RAW)),
    "dist32768": ((1, _D, RAW), (6, _D, GZIP), (9, _D, ZLIB), (6, _F, RAW)),
}


def matrix(pname):
    """the (level, strategy, wrapper) combinations minted for a payload"""
    return THINNED.get(pname) or tuple((lv, st, w) for lv in LEVELS for st in STRATEGIES for w in WRAPS)


def compress(data, level, strategy, wrap):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap], 9, strategy)
    return c.compress(data) + c.flush()


def flush_text():
    return words(300000, 7)


def compress_flushed(data, wrap, every=7000):
    """Z_SYNC_FLUSH every `every` bytes: many blocks, empty stored blocks, window use beyond 32 KiB of output"""
    c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrap])
    out = b""
    for k in range(0, len(data), every):
        out += c.compress(data[k:k + every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


# ---- zlib's verdict -----------------------------------------------------------------------------------------------------------------
def zlib_code(ex):
    m = str(ex)
    if "header" in m or "compression method" in m or "window size" in m or "Error 2 " in m:      # (Error 2: Z_NEED_DICT)
        return HEADER
    if "data check" in m or "length check" in m:
        return CHECKSUM
    assert "invalid" in m or "too many" in m, m
    return CORRUPT


def verdict(wrap, s, cap):
    """(result, bytes) of zlib at capacity cap — o.decompress(s, cap); without eof, o.decompress(o.unconsumed_tail, 1): a byte returned
    is CJ_E_OUT_TOO_SMALL, an exception is that error's code, eof is success (with bytes behind the stream: CJ_E_DEFLATE_TRAILING),
    neither is CJ_E_DEFLATE_EOF.  cap None: no limit.  (max_length 0 means "no limit" to Python: capacity 0 starts at the second step.)"""
    o = zlib.decompressobj(WBITS[wrap])
    s = bytes(s)
    try:
        if cap is None:
            out = o.decompress(s)
        else:
            out, tail = (o.decompress(s, cap), None) if cap > 0 else (b"", s)
            if not o.eof:
                if o.decompress(o.unconsumed_tail if tail is None else tail, 1):
                    return OUT_TOO_SMALL, b""
    except zlib.error as ex:
        return zlib_code(ex), b""
    if not o.eof:
        return EOF, b""
    if o.unused_data:
        return TRAILING, b""
    return len(out), out


def gzip_header_len(s):
    """length of a gzip member's header (one that zlib accepted)"""
    flg, p = s[3], 10
    if flg & 4:
        p += 2 + (s[p] | s[p + 1] << 8)
    for bit in (8, 16):
        if flg & bit:
            p = s.index(b"\0", p) + 1
    return p + (2 if flg & 2 else 0)


def size_verdict(wrap, s):
    """what the size query says: zlib's verdict without a limit, except that the checksums are not verified — a stream whose only fault
    is its checksum has its length (or the error that follows: a trailer cut short, bytes behind it)"""
    r, _ = verdict(wrap, s, None)
    if r != CHECKSUM:
        return r
    s = bytes(s)
    o = zlib.decompressobj(-15)
    out = o.decompress(s[2 if wrap == ZLIB else gzip_header_len(s):])
    assert o.eof
    rest, want = len(o.unused_data), 4 if wrap == ZLIB else 8
    return EOF if rest < want else TRAILING if rest > want else len(out)


# ---- hand-written streams -----------------------------------------------------------------------------------------------------------
class Bits:
    """DEFLATE's bit order: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.b = []

    def put(self, v, n):
        self.b += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, c, n):
        self.b += [(c >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def align(self):
        self.b += [0] * (-len(self.b) % 8)
        return self

    def raw(self, data):
        self.align()
        for x in data:
            self.put(x, 8)
        return self

    def bytes(self):
        b = self.b + [0] * (-len(self.b) % 8)
        return bytes(sum(b[k + j] << j for j in range(8)) for k in range(0, len(b), 8))


def fixed_lit(w, sym):
    if sym < 144:
        return w.code(0x30 + sym, 8)
    if sym < 256:
        return w.code(0x190 + sym - 144, 9)
    if sym < 280:
        return w.code(sym - 256, 7)
    return w.code(0xC0 + sym - 280, 8)


def canon(lens):
    """canonical codes of a (valid or not) set of lengths: symbol -> (code, length)"""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LENS = [4] * 13 + [5] * 6                       # a complete code-length code over all 19 symbols (13/16 + 6/32)


def dyn_header(w, litlens, distlens, final=1, cl_syms=None, nlen=None, ndist=None, cl_lens=None, ncode=19):
    """a dynamic block's header: every code length sent as itself (no repeats) unless cl_syms = [(symbol, extra bits value)] is given;
    cl_lens: the code-length code's own 19 lengths (CL_LENS when None), of which the first ncode in CL_ORDER are sent (HCLEN = ncode - 4)"""
    nlen, ndist = nlen or len(litlens), ndist or len(distlens)
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    w.put(final, 1).put(2, 2).put(nlen - 257, 5).put(ndist - 1, 5).put(ncode - 4, 4)
    for s in CL_ORDER[:ncode]:
        w.put(cl_lens[s], 3)
    cl = canon(cl_lens)
    if cl_syms is None:
        cl_syms = [(l, 0) for l in list(litlens) + list(distlens)]
    for s, x in cl_syms:
        w.code(*cl[s])
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s])
    return w


def _lits(n=258, **kw):
    lens = [0] * n
    for k, v in kw.items():
        lens[int(k[1:])] = v
    return lens


def hand_streams():
    """[(name, wrap, stream)] — what each is for is its name; zlib's verdict on each is recorded by the minter"""
    out = []
    add = lambda name, wrap, s: out.append((name, wrap, bytes(s)))
    hdr = lambda: Bits().put(1, 1).put(1, 2)                                 # final, fixed
    for sym in (286, 287):
        add("fixed_symbol_%d" % sym, RAW, fixed_lit(fixed_lit(hdr(), 97), sym).put(0, 16).bytes())
    for d in (30, 31):
        w = hdr()
        for ch in b"abc":
            fixed_lit(w, ch)
        add("distance_symbol_%d" % d, RAW, fixed_lit(w, 257).code(d, 5).put(0, 16).bytes())
    for d, name in ((2, "distance_equals_produced"), (3, "distance_one_beyond_produced")):
        w = fixed_lit(fixed_lit(hdr(), 97), 98)
        add(name, RAW, fixed_lit(fixed_lit(w, 257).code(d - 1, 5), 256).bytes())
    w = fixed_lit(hdr(), 97)                                                 # a bad distance in a match that would also overrun a small capacity
    add("distance_beyond_and_length_258", RAW, fixed_lit(fixed_lit(w, 285).code(4, 5).put(0, 1), 256).bytes())
    add("length_258_distance_1", RAW, fixed_lit(fixed_lit(fixed_lit(hdr(), 97), 285).code(0, 5), 256).bytes())
    # dynamic headers
    ok_lit = _lits(s97=1, s256=2, s257=2)
    add("repeat_16_first", RAW, dyn_header(Bits(), ok_lit, [1], cl_syms=[(16, 0)] + [(0, 0)] * 20).put(0, 32).bytes())
    add("repeat_overruns", RAW, dyn_header(Bits(), ok_lit, [1], cl_syms=[(18, 127), (18, 127)]).put(0, 32).bytes())
    add("repeat_exact", RAW, dyn_header(Bits(), ok_lit, [1], cl_syms=[(18, 97 - 11), (1, 0), (18, 127), (18, 256 - 236 - 11), (2, 0), (2, 0), (1, 0)])
                             .code(0, 1).code(2, 2).bytes())
    add("too_many_length_symbols", RAW, dyn_header(Bits(), ok_lit, [1], nlen=287).put(0, 64).bytes())
    add("too_many_distance_symbols", RAW, dyn_header(Bits(), ok_lit, [1], ndist=31).put(0, 64).bytes())
    add("oversubscribed_lengths", RAW, dyn_header(Bits(), _lits(s0=1, s1=1, s2=1, s256=2), [1]).put(0, 32).bytes())
    add("oversubscribed_distances", RAW, dyn_header(Bits(), ok_lit, [1, 1, 1]).put(0, 32).bytes())
    add("incomplete_lengths", RAW, dyn_header(Bits(), _lits(s97=2, s256=2), [1]).put(0, 32).bytes())
    add("incomplete_distances", RAW, dyn_header(Bits(), ok_lit, [2, 2]).put(0, 32).bytes())
    add("missing_end_of_block", RAW, dyn_header(Bits(), _lits(s97=1, s98=1), [1]).put(0, 32).bytes())
    # one distance code of length 1: legal; its sibling code is not a symbol
    w = dyn_header(Bits(), ok_lit, [1]).code(0, 1).code(3, 2).code(0, 1).code(2, 2)           # 'a', length 3, distance 1, end
    add("single_distance_code", RAW, w.bytes())
    w = dyn_header(Bits(), ok_lit, [1]).code(0, 1).code(3, 2).code(1, 1).code(2, 2)
    add("single_distance_code_unused_sibling", RAW, w.bytes())
    add("no_distance_code_literals_only", RAW, dyn_header(Bits(), ok_lit, [0]).code(0, 1).code(0, 1).code(2, 2).bytes())
    add("no_distance_code_but_a_match", RAW, dyn_header(Bits(), ok_lit, [0]).code(0, 1).code(3, 2).put(0, 16).bytes())
    add("single_length_code_end_only", RAW, dyn_header(Bits(), _lits(s256=1), [0]).code(0, 1).bytes())
    add("single_length_code_unused_sibling", RAW, dyn_header(Bits(), _lits(s256=1), [0]).code(1, 1).put(0, 8).bytes())
    # a code-length code without a single code: inflate reads every length as 0, one bit each, and misses the end-of-block code
    w = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(0, 12)
    add("no_code_length_code", RAW, w.put(0, 300).bytes())
    add("no_code_length_code_cut", RAW, w.bytes()[:20])
    add("incomplete_code_length_code", RAW, Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 9).put(0, 64).bytes())
    # stored blocks, block type 3
    add("stored_len_mismatch", RAW, Bits().put(1, 1).put(0, 2).raw(b"\x03\x00\xfc\xfe" + b"abc").bytes())
    add("stored_ok", RAW, Bits().put(1, 1).put(0, 2).raw(b"\x03\x00\xfc\xff" + b"abc").bytes())
    add("stored_empty_then_fixed", RAW, fixed_lit(fixed_lit(Bits().put(0, 1).put(0, 2).raw(b"\x00\x00\xff\xff").put(1, 1).put(1, 2), 120), 256).bytes())
    add("stored_cut_in_data", RAW, Bits().put(1, 1).put(0, 2).raw(b"\x10\x00\xef\xff" + b"abcdefgh").bytes())
    add("block_type_3", RAW, Bits().put(1, 1).put(3, 2).put(0, 29).bytes())
    add("block_type_3_after_a_block", RAW, fixed_lit(fixed_lit(Bits().put(0, 1).put(1, 2), 97), 256).put(1, 1).put(3, 2).put(0, 16).bytes())
    # a valid stream cut at every byte: the header, inside a table, inside a symbol, inside extra bits, inside the trailer
    text = words(300, 5)
    for wrap in WRAPS:
        s = compress(text, 9, zlib.Z_DEFAULT_STRATEGY, wrap)
        for k in range(len(s)):
            add("%s_cut_%03d" % (WRAP_NAME[wrap], k), wrap, s[:k])
    s = compress(words(2000, 6), 1, zlib.Z_FIXED, RAW)
    for k in range(0, len(s), 37):
        add("raw_fixed_cut_%04d" % k, RAW, s[:k])
    # zlib headers and trailers
    body = compress(text, 6, zlib.Z_DEFAULT_STRATEGY, RAW)
    adler = zlib.adler32(text).to_bytes(4, "big")
    zh = lambda cmf, flg: bytes([cmf, flg + (31 - (cmf * 256 + flg) % 31) % 31])
    add("zlib_ok_window_256", ZLIB, zh(0x08, 0) + body + adler)
    add("zlib_cm_7", ZLIB, zh(0x77, 0) + body + adler)
    add("zlib_cinfo_8", ZLIB, zh(0x88, 0) + body + adler)
    add("zlib_bad_fcheck", ZLIB, bytes([0x78, 0x9d]) + body + adler)
    add("zlib_fdict", ZLIB, zh(0x78, 0x20) + b"\x01\x02\x03\x04" + body + adler)
    add("zlib_fdict_cut", ZLIB, zh(0x78, 0x20) + b"\x01\x02")
    add("zlib_bad_adler", ZLIB, zh(0x78, 0x80) + body + bytes([adler[0] ^ 1]) + adler[1:])
    add("zlib_trailing_byte", ZLIB, zh(0x78, 0x80) + body + adler + b"\0")
    add("zlib_two_streams", ZLIB, (zh(0x78, 0x80) + body + adler) * 2)
    # gzip headers and trailers
    crc, isize = zlib.crc32(text).to_bytes(4, "little"), len(text).to_bytes(4, "little")
    gz = lambda flg, extra=b"", cm=8, magic=b"\x1f\x8b": magic + bytes([cm, flg]) + b"\x00\x01\x02\x03\x02\x03" + extra
    hcrc = lambda h: h + (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    fields = b"\x05\x00EXTRA" + b"name.txt\0" + b"a comment\0"
    add("gzip_plain", GZIP, gz(0) + body + crc + isize)
    add("gzip_bad_magic", GZIP, gz(0, magic=b"\x1f\x8c") + body + crc + isize)
    add("gzip_cm_7", GZIP, gz(0, cm=7) + body + crc + isize)
    for bit in (0x20, 0x40, 0x80):
        add("gzip_reserved_flag_%02x" % bit, GZIP, gz(bit) + body + crc + isize)
    add("gzip_ftext", GZIP, gz(1) + body + crc + isize)
    add("gzip_fhcrc", GZIP, hcrc(gz(2)) + body + crc + isize)
    add("gzip_bad_fhcrc", GZIP, gz(2) + b"\x12\x34" + body + crc + isize)
    add("gzip_all_four_fields", GZIP, hcrc(gz(0x1e, fields)) + body + crc + isize)
    add("gzip_all_four_fields_bad_fhcrc", GZIP, gz(0x1e, fields) + b"\x00\x00" + body + crc + isize)
    add("gzip_fextra_fname", GZIP, gz(0x0c, b"\x00\x00" + b"n\0") + body + crc + isize)
    add("gzip_long_fextra", GZIP, gz(4, b"\x00\x03" + bytes(768)) + body + crc + isize)
    add("gzip_fextra_cut", GZIP, gz(4, b"\x40\x00" + bytes(10)))
    add("gzip_fname_unterminated", GZIP, gz(8, b"name without end"))
    add("gzip_bad_crc", GZIP, gz(0) + body + bytes([crc[0] ^ 0x80]) + crc[1:] + isize)
    add("gzip_bad_isize", GZIP, gz(0) + body + crc + bytes([isize[0] ^ 1]) + isize[1:])
    add("gzip_bad_crc_isize_cut", GZIP, gz(0) + body + bytes([crc[0] ^ 0x80]) + crc[1:] + isize[:2])
    add("gzip_trailing_byte", GZIP, gz(0) + body + crc + isize + b"\0")
    add("gzip_second_member", GZIP, (gz(0) + body + crc + isize) * 2)
    # raw: bytes behind the byte that holds the final block's last bit
    add("raw_trailing_byte", RAW, body + b"\0")
    add("raw_trailing_stream", RAW, body + body)
    add("empty_input_raw", RAW, b"")
    return out


# ---- the committed fixtures -----------------------------------------------------------------------------------------------------------
_cache = {}


def _load():
    if "meta" not in _cache:
        with open(os.path.join(GOLDEN, "golden_deflate.json")) as f:
            meta = json.load(f)
        # the compact rows of the minter, expanded
        empty = sha(b"")
        valid, off = [], 0
        for name, ln, n, h in meta["valid"]:
            payload, lv, st, wr = name.split("_") if name.count("_") == 3 else (name.split("_")[0], "l6", "default", name.split("_")[1])
            valid.append(dict(name=name, wrap=("raw", "zlib", "gzip").index(wr), off=off, len=ln, result=n, n=n, sha256=h, payload=payload, level=int(lv[1:]), strategy=st))
            off += ln
        meta["valid"] = valid
        names = [v["name"] for v in valid]
        meta["mutations"] = [dict(name="mut%03d_%s" % (k, names[b]), base=names[b], bit=bit, cut=cut, cap=meta["valid"][b]["n"] + meta["mutation_slack"],
                                  result=r, n=n, sha256=h or empty) for k, (b, bit, cut, r, n, h) in enumerate(meta["mutations"])]
        meta["hand"] = [dict(name=name, cap=meta["hand_cap"], result=r, n=n, sha256=h or empty) for name, r, n, h in meta["hand"]]
        _cache["meta"] = meta
        with open(os.path.join(GOLDEN, "golden_deflate.bin"), "rb") as f:
            _cache["bin"] = f.read()
    return _cache["meta"], _cache["bin"]


def valid():
    """the minted streams: name, wrap, bytes, result (= n, zlib's verdict at capacity n), n, sha256, cap = n"""
    if "valid" not in _cache:
        meta, blob = _load()
        _cache["valid"] = [dict(v, bytes=blob[v["off"]:v["off"] + v["len"]], cap=v["n"]) for v in meta["valid"]]
    return _cache["valid"]


def flip(s, bit):
    m = bytearray(s)
    m[bit >> 3] ^= 1 << (bit & 7)
    return bytes(m)


def mutations():
    """single-bit flips (bit) / cuts (cut) of fixture streams with zlib's verdict at cap"""
    if "mut" not in _cache:
        meta, _ = _load()
        by = {v["name"]: v for v in valid()}
        ms = []
        for m in meta["mutations"]:
            base = by[m["base"]]
            s = flip(base["bytes"], m["bit"]) if m["cut"] is None else base["bytes"][:m["cut"]]
            ms.append(dict(m, wrap=base["wrap"], bytes=s))
        _cache["mut"] = ms
    return _cache["mut"]


def hand():
    """the hand-written streams with zlib's verdict (result, n, sha256) at cap, as the minter recorded it"""
    if "hand" not in _cache:
        meta, _ = _load()
        hs = hand_streams()
        assert [h[0] for h in hs] == [m["name"] for m in meta["hand"]], "tests/golden/golden_deflate.json is stale: run tests/golden/make_golden_deflate.py"
        _cache["hand"] = [dict(m, wrap=h[1], bytes=h[2]) for h, m in zip(hs, meta["hand"])]
    return _cache["hand"]


def _load_others():
    if "ometa" not in _cache:
        with open(os.path.join(GOLDEN, "golden_deflate_others.json")) as f:
            _cache["ometa"] = json.load(f)
        with open(os.path.join(GOLDEN, "golden_deflate_others.bin"), "rb") as f:
            _cache["obin"] = f.read()
    return _cache["ometa"], _cache["obin"]


def others():
    """the streams libdeflate and zopfli wrote (tests/golden/make_golden_deflate_others.py): name = payload_encoder_wrapper, wrap, bytes,
    result = n = cap (zlib's verdict at capacity n), sha256"""
    if "others" not in _cache:
        meta, blob = _load_others()
        out, off = [], 0
        for name, ln, n, h in meta["valid"]:
            payload, enc, wr = name.split("_")
            out.append(dict(name=name, wrap=("raw", "zlib", "gzip").index(wr), bytes=blob[off:off + ln], len=ln, result=n, n=n, cap=n, sha256=h, payload=payload, encoder=enc))
            off += ln
        assert off == len(blob)
        _cache["others"] = out
    return _cache["others"]


def other_mutations():
    """single-bit flips and cuts of four of them with zlib's verdict at cap"""
    if "omut" not in _cache:
        meta, _ = _load_others()
        vs, empty = others(), sha(b"")
        ms = []
        for k, (b, bit, cut, r, n, h) in enumerate(meta["mutations"]):
            base = vs[b]
            s = flip(base["bytes"], bit) if cut is None else base["bytes"][:cut]
            ms.append(dict(name="omut%03d_%s" % (k, base["name"]), base=base["name"], wrap=base["wrap"], bytes=s, bit=bit, cut=cut, cap=base["n"] + meta["mutation_slack"],
                           result=r, n=n, sha256=h or empty))
        _cache["omut"] = ms
    return _cache["omut"]


def cases(wrap=None):
    cs = valid() + mutations() + hand()
    return cs if wrap is None else [c for c in cs if c["wrap"] == wrap]


# ---- the kernel's decoder on the host ---------------------------------------------------------------------------------------------------
def sim_lib():
    if "sim" not in _cache:
        L = C.CDLL(build_sim("sim_deflate_decode.cpp", os.path.join(SIM_DIR, "libsim_deflate_decode.so")))
        L.sim_deflate_decode.restype = C.c_longlong
        L.sim_deflate_decode.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
        _cache["sim"] = L
    return _cache["sim"]


def sim_decode(wrap, s, cap, mis=0, size=False):
    """(result, bytes) of the host build; the stream lies `mis` bytes behind a 16-byte boundary"""
    L = sim_lib()
    buf = (C.c_ubyte * (len(s) + 32))()
    at = C.addressof(buf) + (-C.addressof(buf)) % 16 + mis
    C.memmove(at, bytes(s), len(s))
    out = (C.c_ubyte * max(cap, 1))()
    r = L.sim_deflate_decode(wrap, 1 if size else 0, at, len(s), out, cap)
    return r, (bytes(out[:r]) if r > 0 and not size else b"")


def device_call(e, N, wrap, chunks, caps, sizes=False):
    """cj_deflate_batch_device (sizes: cj_deflate_batch_sizes_device) in the harness's guarded run (tests/device_batch.py): chunks at
    every misalignment, 64 guard bytes around every slot, the output filled with 0xA5 first: (results, output, offsets)"""
    import device_batch as DB
    n, L = len(chunks), N.lib()
    if sizes:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_sizes_device(e.h, wrap, 0, n, i, o, l, r, None))
    else:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(e.h, wrap, N.OP_DECOMPRESS, 0, n, i, o, l, out, oo, oc, r, None))
    return DB.run_chunks(e, call, chunks, caps)
