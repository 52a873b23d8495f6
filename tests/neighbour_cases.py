"""What lies around a chunk in memory (tests/test_neighbours_model.py on the CPU, tests/test_neighbours_gpu.py on the GPU; DESIGN.md
5.10a): one layout function that packs a batch's inputs under a *ring* — the bytes in front of and behind every chunk — and the case
lists of every decoder and encoder that reads a batch.  The property held: a chunk's result and output bytes are a function of its own
in_len bytes, its capacity and its dictionary, and of nothing else in memory; so every case has ONE expected value, computed by the
codec's reference on the chunk alone, and every ring must give it.

  zero     0x00 in front and behind, 16 bytes or more of gap: the layout of the older tests (the control)
  ff       64 bytes of 0xFF on both sides
  own      in front the chunk's own last 64 bytes; behind a decoder's chunk the stream's own continuation s[k:k + 64] (an uncut stream:
           its head again), behind an encoder's input the bytes that continue its period
  packed   no gap at all: chunk i + 1 begins where chunk i ends, in an order shuffled by a fixed seed, 64 bytes of 0xFF at both ends

Every blob keeps 64 bytes of margin at both ends: a read a few bytes outside a chunk stays inside the allocation.  Expected values
come from zlib (live), libzstd (recorded: tests/golden/golden_neighbours.json), the Python models and the encoders' C models — never
from a GPU path.  No GPU needed to import this."""
import functools
import hashlib
import json
import os
import zlib

import numpy as np

import deflate_cases as DF
import device_batch as DB

M = 64                                             # ring bytes on each side, and the blob's margin
RINGS = ("zero", "ff", "own", "packed")
ROOMS = (0, 64)                                    # capacities U and U + 64
GOLDEN_JSON = os.path.join(DF.GOLDEN, "golden_neighbours.json")


# ---- the layout -------------------------------------------------------------------------------------------------------------------------
def layout(chunks, ring, own=None, mis=None, seed=20):
    """(blob, offsets, fronts, behinds): the chunks packed under `ring`.  own[i] = (front, behind), 64 bytes each (the `own` ring);
    mis[i] = the chunk's offset modulo 16 ((5 i) mod 16 when None; `packed` has the offsets its chunks' lengths give).  fronts[i] and
    behinds[i] are the 64 bytes that lie in front of and behind chunk i in the blob, whatever put them there: what a model is shown."""
    n = len(chunks)
    off = np.zeros(n, np.uint64)
    if ring == "packed":
        run = M
        for i in np.random.default_rng(seed).permutation(n):
            off[i] = run; run += len(chunks[i])
        blob = np.full(run + M, 0xFF, np.uint8)
    else:
        assert ring in RINGS
        run = 0
        for i, c in enumerate(chunks):
            off[i] = run + M + ((5 * i) % 16 if mis is None else mis[i] % 16)
            run = (int(off[i]) + len(c) + M + 15) // 16 * 16 + 16
        blob = np.zeros(run + M, np.uint8)
    for i, c in enumerate(chunks):
        o = int(off[i])
        if ring == "ff":
            blob[o - M:o + len(c) + M] = 0xFF
        elif ring == "own":
            f, b = own[i]
            assert len(f) == M and len(b) == M
            blob[o - M:o] = np.frombuffer(f, np.uint8)
            blob[o + len(c):o + len(c) + M] = np.frombuffer(b, np.uint8)
        blob[o:o + len(c)] = np.frombuffer(c, np.uint8)
    fronts = [blob[int(o) - M:int(o)].tobytes() for o in off]
    behinds = [blob[int(o) + len(c):int(o) + len(c) + M].tobytes() for o, c in zip(off, chunks)]
    return blob, off, fronts, behinds


_layouts = {}


def case_layout(key, cases, ring):
    """layout() of a case list, built once per (key, ring)"""
    if (key, ring) not in _layouts:
        _layouts[(key, ring)] = layout([c["bytes"] for c in cases], ring, [c["own"] for c in cases], [c["mis"] for c in cases])
    return _layouts[(key, ring)]


def _tile(src, n):
    src = src or b"\xff"
    return src * (n // len(src) + 1)


def own_of_cut(s, k):
    """the `own` ring of a decoder's chunk s[:k]: its own last 64 bytes (a shorter chunk: behind the stream's) | the continuation"""
    return (_tile(s, M) + s[:k])[-M:], (s[k:] + _tile(s, M))[:M]


def _case(base, s, k, cap, result, i, out=None, sha=None, **extra):
    f, b = own_of_cut(s, k)
    return dict(extra, base=base, k=k, bytes=s[:k], cap=cap, result=int(result), out=out, sha=sha, own=(f, b), mis=(5 * i) % 16)


def at_four_alignments(cases):
    """every case four times: offsets 0, 1, 2 and 3 modulo 4, and all sixteen modulo 16 over any four cases in a row"""
    return [dict(c, mis=j + 4 * ((i + j) % 4)) for i, c in enumerate(cases) for j in range(4)]


# ---- decoders: DEFLATE, zlib, gzip ------------------------------------------------------------------------------------------------------
DEFLATE_RECIPES = (("l9_default", 9, zlib.Z_DEFAULT_STRATEGY), ("l1_fixed", 1, zlib.Z_FIXED), ("l0_stored", 0, zlib.Z_DEFAULT_STRATEGY),
                   ("l6_huff", 6, zlib.Z_HUFFMAN_ONLY))


@functools.lru_cache(maxsize=None)
def deflate_bases(wrap):
    text = DF.words(300, 5)
    out = [("%s_%s" % (DF.WRAP_NAME[wrap], name), DF.compress(text, lv, st, wrap)) for name, lv, st in DEFLATE_RECIPES]
    assert all(len(s) <= 400 for _, s in out)
    return out


@functools.lru_cache(maxsize=None)
def _deflate_cuts(wrap):
    out = []
    for base, s in deflate_bases(wrap):
        for k in range(len(s) + 1):
            size = DF.size_verdict(wrap, s[:k])
            for room in ROOMS:
                r, o = DF.verdict(wrap, s[:k], 300 + room)
                out.append(_case(base, s, k, 300 + room, r, len(out), out=o, size=size, wrap=wrap))
    return out


@functools.lru_cache(maxsize=None)
def deflate_cases(wrap):
    """every cut of four zlib-written streams at capacities U and U + 64, zlib's live verdict on s[:k]; `size`: the size query's"""
    return at_four_alignments(_deflate_cuts(wrap))


@functools.lru_cache(maxsize=None)
def deflate_size_cases(wrap):
    """the same cuts for the size query: result = deflate_cases.size_verdict, no output (`sized`)"""
    return at_four_alignments([dict(c, result=c["size"], sized=True, cap=0, out=None) for c in _deflate_cuts(wrap) if c["cap"] == 300])


# ---- decoders: Zstandard (recorded) -----------------------------------------------------------------------------------------------------
# (frame:checksum / nochecksum, frame:fcs / nofcs, lit:huf1, lit:raw, block:rle, a two-frame chunk; ll:fse: the smallest fixture that
# shows it has 532 bytes, every other base at most 400)
ZSTD_BASES = ("text_300", "period7", "hand_rle_repeat", "hand_nseq_127", "two_frames", "small_alphabet")


def zstd_base_streams():
    import zstd_cases as Z
    by = {c.name: c for c in Z.load_cases()}
    return [(name, by[name].stream, by[name].cap) for name in ZSTD_BASES]


def mint_zstd():
    """the document of tests/golden/golden_neighbours.json from the libzstd that is loaded (tests/golden/make_golden_neighbours.py)"""
    import zstd_cases as Z
    doc = {"libzstd": Z.libzstd().ZSTD_versionString().decode(), "rooms": list(ROOMS), "bases": []}
    for name, s, U in zstd_base_streams():
        results, shas = [[] for _ in ROOMS], {}
        for k in range(len(s) + 1):
            for j, room in enumerate(ROOMS):
                r, o = Z.zstd_verdict(s[:k], U + room)
                results[j].append(r)
                if r >= 0:
                    assert shas.setdefault(str(k), Z.sha(o)) == Z.sha(o)
        doc["bases"].append({"name": name, "len": len(s), "cap": U, "results": results, "sha256": shas})
    return doc


@functools.lru_cache(maxsize=None)
def zstd_doc():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def zstd_cases():
    """every cut of six recorded frames at capacities U and U + 64 with libzstd's recorded verdict (sha256 where it accepts)"""
    doc, out = zstd_doc(), []
    assert [b["name"] for b in doc["bases"]] == list(ZSTD_BASES) and doc["rooms"] == list(ROOMS)
    for (name, s, U), b in zip(zstd_base_streams(), doc["bases"]):
        assert len(s) == b["len"] and U == b["cap"], "tests/golden/golden_neighbours.json is stale: run tests/golden/make_golden_neighbours.py"
        for k in range(len(s) + 1):
            for j, room in enumerate(ROOMS):
                out.append(_case(name, s, k, U + room, b["results"][j][k], len(out), sha=b["sha256"].get(str(k))))
    return at_four_alignments(out)


# ---- decoders: LZ4 against a dictionary --------------------------------------------------------------------------------------------------
DICT_LEN = 4096
DICT_TAILS = ((None, 13), (19, 6))


@functools.lru_cache(maxsize=None)
def lz4_dict_cases():
    """family A of tests/input_cases.py (cuts at both ends and around eight tokens) on bodies a and b whose first matches reach into a
    4 096-byte dictionary; tests/lz4_dict_model.py decides"""
    import capacity_cases as K
    import input_cases as I
    import lz4_dict_model as D
    d, out = D.dictionary(DICT_LEN), []
    for body in ("a", "b"):
        for s in I._pick(K.lz4_streams(body, DICT_LEN), DICT_TAILS):
            full, tok = s["bytes"], I.lz4_tokens(s["seqs"])
            for k in I.cut_lens(len(full), [tok[j][0] for j in K.CUTS]):
                for room in ROOMS:
                    r, o = D.decode(full[:k], s["U"] + room, d)
                    out.append(_case("%s/%s" % (body, s["name"]), full, k, s["U"] + room, r, len(out), out=o))
    return out


# ---- decoders: BGZF ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bgzf_bases():
    import bgzf_model as B
    return (("two", B.stream([b"hello, blocked gzip", B._text(90, 41)], marker=False)),
            ("three", B.stream([B._text(3000, 51), B._text(2000, 52), B._text(1000, 53)], 9)))


@functools.lru_cache(maxsize=None)
def bgzf_cases():
    """the two-member and the three-member stream cut at every byte at capacities U and U + 64: the model's verdict, and `size`"""
    import bgzf_model as B
    out = []
    for base, s in bgzf_bases():
        U = B.sizes(s)
        for k in range(len(s) + 1):
            size = B.sizes(s[:k])
            for room in ROOMS:
                r, o = B.decode(s[:k], U + room)
                out.append(_case(base, s, k, U + room, r, len(out), out=o, size=size))
    return out


@functools.lru_cache(maxsize=None)
def bgzf_size_cases():
    """one case per cut of the same streams for the size query and the walk — result = the ISIZE sum or the walk's error, no output
    (`sized`) —, each at offsets 0, 1, 2 and 3 modulo 4"""
    cuts = [c for c in bgzf_cases() if c["cap"] == max(x["cap"] for x in bgzf_cases() if x["base"] == c["base"])]
    return at_four_alignments([dict(c, result=c["size"], sized=True, cap=0, out=None) for c in cuts])


def alignment_coverage(cases, off):
    """what the issue asks of a batch's offsets: all sixteen values modulo 16 over the batch, and all four modulo 4 for every base
    stream with sixteen cases or more; returns the offending (base, values) pairs, [] when the batch complies"""
    by = {}
    for c, o in zip(cases, off):
        by.setdefault(c["base"], set()).add(int(o) % 16)
    bad = [(b, sorted(s)) for b, s in by.items() if sum(1 for c in cases if c["base"] == b) >= 16 and {m % 4 for m in s} != {0, 1, 2, 3}]
    if len(cases) >= 64 and len(set().union(*by.values())) != 16:
        bad.append(("batch", sorted(set().union(*by.values()))))
    return bad


# ---- decoders: Blosc chunks with BloscLZ, Zlib and Zstd streams -----------------------------------------------------------------------------
def _whole(name, chunk, cap, result, i, **extra):
    return _case(name, chunk, len(chunk), cap, result, i, **extra)


@functools.lru_cache(maxsize=None)
def blosc_cases(which):
    """(flags, cases): the fixture, malformed and hand-written chunks of tests/blosclz_model.py ("blosclz") or
    tests/blosc_zcodec_model.py ("zcodecs"), whole, with the models' own expected values; `written`: the bytes of its slot a chunk may
    have written (the result where accepted, the capacity behind a stream found bad, nothing behind a refusal from the header)"""
    import blosc_model as BM
    out = []
    if which == "blosclz":
        import blosclz_model as Z
        flags = Z.FLAG
        for v in Z.valid():
            out.append(_whole(v["name"], v["bytes"], v["nbytes"], v["nbytes"], len(out), sha=v["sha256"], written=v["nbytes"]))
        more = [(m, 70000) for m in Z.malformed()] + [(h, int.from_bytes(h["bytes"][4:8], "little")) for h in Z.hand_chunks()]
        for h, cap in more:
            if h["verdict"] == "ok":
                want = h["out"] if h.get("out") is not None else Z.decode(h["bytes"])
                out.append(_whole(h["name"], h["bytes"], cap, len(want), len(out), out=want, written=len(want)))
            else:
                out.append(_whole(h["name"], h["bytes"], cap, BM.CODE[h["verdict"]], len(out), written=cap if h["verdict"] == BM.CORRUPT else 0))
    else:
        import blosc_zcodec_model as Z
        flags = 2 | Z.FLAGS
        for v in Z.valid():
            out.append(_whole(v["name"], v["bytes"], v["nbytes"], v["nbytes"], len(out), sha=v["sha256"], written=v["nbytes"]))
        for c in Z.malformed() + Z.hand():
            if c["verdict"] == "ok":
                out.append(_whole(c["name"], c["bytes"], c["cap"], c["nbytes"], len(out), sha=c["sha256"], written=c["nbytes"]))
            else:
                out.append(_whole(c["name"], c["bytes"], c["cap"], BM.CODE[c["verdict"]], len(out), written=c["cap"] if c["verdict"] == BM.CORRUPT else 0))
    return flags, out


# ---- decoders: LZ4 / Snappy blocks, the front side -------------------------------------------------------------------------------------------
FRONT = 48


@functools.lru_cache(maxsize=None)
def front_cases(codec):
    """the `own` cases of family A, body a (tests/input_cases.py) as cases of layout()'s `own` ring"""
    import input_cases as I
    cs = I.a_lz4_cases("a") if codec == "lz4" else I.a_snappy_cases("a")
    assert all(len(c["after"]) <= M for c in cs)
    # for layout()'s `own` ring: FRONT bytes of 0xFF in front, the case's own `after` (the stream's continuation) behind, zeros beyond
    return [dict(c, base=c["stream"], k=c["in_len"], sha=None, mis=(5 * i) % 16,
                 own=(bytes(M - FRONT) + b"\xff" * FRONT, c["after"] + bytes(M - len(c["after"]))))
            for i, c in enumerate(c for c in cs if c["kind"] == "own")]


# ---- encoders -------------------------------------------------------------------------------------------------------------------------------
PERIODS = (1, 2, 3, 4, 7, 8, 16, 31, 64)
LENGTHS = tuple(range(1, 41)) + (63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536)


def _pattern(p):
    """p bytes, no two neighbours equal (so that the period is p and not a divisor's, p = 1 aside)"""
    g = DF._lcg(900 + p)
    out = []
    while len(out) < p:
        b = next(g) & 0xFF
        if not out or (b != out[-1] and (len(out) < p - 1 or b != out[0])):
            out.append(b)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def encoder_inputs():
    """periodic data of every period and length, flanked (ring `own`) by the bytes that the period produces before position 0 and behind
    n; and word-like text of every length, behind it its own last 32 bytes twice, in front its own last 64"""
    out = []
    for p in PERIODS:
        pat = _pattern(p)
        phase = p // 3
        at = lambda lo, hi: bytes(pat[(j + phase) % p] for j in range(lo, hi))
        long = at(-M, max(LENGTHS) + M)
        for n in LENGTHS:
            out.append(dict(name="period%d_len%d" % (p, n), base="period%d" % p, period=p, bytes=long[M:M + n], own=(long[:M], long[M + n:M + n + M]), mis=(5 * len(out)) % 16))
    text = DF.words(max(LENGTHS), 25)
    for n in LENGTHS:
        t = text[:n]
        out.append(dict(name="words_len%d" % n, base="words", period=0, bytes=t, own=(_tile(t, M)[-M:], (_tile(t[-32:], M))[:M]), mis=(5 * len(out)) % 16))
    return out


ENCODERS = ("lz4", "snappy", "lz4_dict", "deflate_raw", "deflate_zlib", "deflate_gzip", "zstd")
_enc = {}


def encoder_expected(codec):
    """[(capacity, the model's stream)] per input of encoder_inputs(): tests/hostsim/enc2_model.c (lz4, snappy), enc2_linked_model.c with
    the dictionary as history (lz4_dict), deflate_enc_model.c, zstd_enc_model.c — on the input alone"""
    if codec in _enc:
        return _enc[codec]
    from cramjam_amd import _native as N                                     # (the bounds: host functions of the library)
    raws = [c["bytes"] for c in encoder_inputs()]
    _lz4_bound = lambda n: N.lib().cj_lz4_block_compress_bound(n, 0)
    if codec in ("lz4", "snappy"):
        from test_enc2_model import model_lib, model_lz4, model_snappy
        L = model_lib()
        want = [model_lz4(L, r) if codec == "lz4" else model_snappy(L, r) for r in raws]
        caps = [_lz4_bound(len(r)) if codec == "lz4" else N.lib().cj_snappy_raw_max_compress_len(len(r)) for r in raws]
    elif codec == "lz4_dict":
        import lz4_dict_model as D
        from test_enc2_linked_model import linked_lib, model_linked
        L, d = linked_lib(), D.dictionary(DICT_LEN)
        want = [model_linked(L, d, r) for r in raws]
        caps = [_lz4_bound(len(r)) for r in raws]
    elif codec.startswith("deflate"):
        import deflate_enc_cases as E
        wrap = ("deflate_raw", "deflate_zlib", "deflate_gzip").index(codec)
        want = [E.model(r, wrap)[1] for r in raws]
        caps = [E.bound(len(r), wrap) for r in raws]
    else:
        import zstd_enc_cases as E
        want = [E.model(r, 0)[1] for r in raws]
        caps = [E.bound(len(r), 0) for r in raws]
    assert all(0 < len(w) <= c for w, c in zip(want, caps))
    _enc[codec] = list(zip(caps, want))
    return _enc[codec]


def encoder_cases(codec):
    """encoder_inputs() as cases: result = the length of the model's stream, out = its bytes, cap = the codec's bound"""
    return [dict(c, cap=cap, result=len(w), out=w, sha=None) for c, (cap, w) in zip(encoder_inputs(), encoder_expected(codec))]


# ---- what the GPU suites that run these cases share (tests/test_neighbours_gpu.py, tests/test_scratch_contents_gpu.py) -----------------
sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()


def tag(key, ring, c, got):
    return key, ring, c["base"], "k", c.get("k"), "len", len(c["bytes"]), "cap", c["cap"], "got", int(got), "want", c["result"]


def device(e, key, cases, ring, call, packed=None, dictionary=None, more=0):
    """one device batch on the harness (tests/device_batch.py): call(d_in, in_off, in_len, d_out, out_off, out_cap, result[, d_dict])
    over the cases packed under `ring` (packed: a (blob, offsets) made elsewhere; more: bytes added to every in_len), then every
    assertion of tests/test_neighbours_gpu.py's head; returns (results, output, slot offsets)"""
    blob, off = packed if packed is not None else case_layout(key, cases, ring)[:2]
    assert not alignment_coverage(cases, off), (key, ring, alignment_coverage(cases, off))
    return DB.run_cases(e, key, cases, call, lambda i, got: tag(key, ring, cases[i], got), packed=(blob, off), more=more, dictionary=dictionary,
                        with_input=True, what="a guard byte or a byte behind the result changed")


def shuffled(cases, seed=20):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


def host_check(key, cases, res, outs):
    for c, r, o in zip(cases, res, outs):
        assert r == c["result"], tag(key, "host", c, r)
        assert len(o) == max(r, 0) and (r <= 0 or ((bytes(o) == c["out"]) if c["out"] is not None else (sha(o) == c["sha"]))), ("bytes", tag(key, "host", c, r))


def bgzf_decode_cases():
    """a refused BGZF stream is refused by the walk or for its capacity before a byte is written, or by a member's decoder, which may
    have written inside the slot"""
    return [dict(c, written=0 if c["size"] < 0 or c["size"] > c["cap"] else c["cap"]) for c in bgzf_cases()]


def encode_call(eng, codec, n):
    from cramjam_amd import _native as N
    L = N.lib()
    if codec in ("lz4", "snappy"):
        return lambda i, o, l, out, oo, oc, r: eng.batch_device(N.CODEC_LZ4_BLOCK if codec == "lz4" else N.CODEC_SNAPPY_RAW, N.OP_COMPRESS, 0, n, i, o, l, out, oo, oc, r)
    if codec == "lz4_dict":
        return lambda i, o, l, out, oo, oc, r, d: N.check(L.cj_dict_batch_device(eng.h, N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, 0, n, i, o, l, out, oo, oc, r, d, DICT_LEN, None))
    if codec.startswith("deflate"):
        wrap = ENCODERS.index(codec) - 3
        return lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_compress_batch_device(eng.h, wrap, 0, n, i, o, l, out, oo, oc, r, None))
    return lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_compress_batch_device(eng.h, N.ZSTD_FRAMES, 0, n, i, o, l, out, oo, oc, r, None))
