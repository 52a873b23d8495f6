"""The case lists of the far placement (tests/device_batch.py: run_far; tests/test_far_offsets_gpu.py on the GPU, tests/test_far_cases_model.py
on the CPU): one list per device entry and direction, every one a SUBSET of a list the suite already has — chosen by a fixed stride,
at most 64 cases per place —, so every expected result and byte is already the reference's: the CPU oracle, zlib, the recorded
libzstd verdicts, the Python models, the encoders' C models, the golden ORC and Parquet files.  Nothing is minted here but subsets.

A list is a dict: cases (dicts as tests/device_batch.py describes them), call(eng) -> the function run_far calls with (idx, d_in,
in_off, in_len, d_out, out_off, out_cap, result[, d_dict]) — idx: the cases of this call as indices of the list —, refuses (the entry
can refuse a chunk: the list then holds a refused case), encoder (place B then holds an input of 1 KiB or more), dictionary.
LISTS maps a name to its builder; far_list(name) builds once.  No GPU is needed to import this or to build a list."""
import functools

import numpy as np

PER_PLACE = 16
LISTS = {}


def _stride(cases, n):
    return cases[::max(1, len(cases) // n)][:n] if n > 0 else []


def pick(cases, per_place=PER_PLACE):
    """4 x per_place cases (or all, when there are fewer): the accepted cases with output at one fixed stride, the others at another —
    a cut sweep is refusals almost everywhere —, dealt in fours so that every place gets both kinds"""
    cases, n = list(cases), 4 * per_place
    ok = lambda c: c["result"] is None or c["result"] > 0
    acc, rej = [c for c in cases if ok(c)], [c for c in cases if not ok(c)]
    na = max(min(len(acc), n // 2), n - len(rej))
    acc, rej = _stride(acc, na), _stride(rej, n - na)
    out = []
    while acc or rej:
        out += acc[:4] + rej[:4]
        acc, rej = acc[4:], rej[4:]
    return out


def sized(c, result):
    """the case of a size query: no output, capacity 0"""
    return dict(c, result=int(result), cap=0, sized=True, out=None, sha=None)


def _list(name, **kw):
    def deco(fn):
        LISTS[name] = functools.partial(fn, **kw) if kw else fn
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def far_list(name):
    d = LISTS[name]()
    d.setdefault("dictionary", None)
    d.setdefault("encoder", False)
    d.setdefault("refuses", True)
    d["name"] = name
    return d


def tag_of(name):
    cs = far_list(name)["cases"]
    return lambda i, got: (name, "case", i, "place", "ABCD"[i % 4], "len", len(cs[i]["bytes"]), "cap", cs[i]["cap"], "got", got, "want", cs[i]["result"])


def _native():
    from cramjam_amd import _native as N
    return N, N.lib()


# ---- LZ4 / Snappy blocks -------------------------------------------------------------------------------------------------------------------------
def _block_cases(codec):
    import capacity_cases as K
    if codec == "lz4":
        return pick([c for body in K.LZ4_BODIES[:2] for c in K.lz4_cases(body)])          # (bodies a and b: every window decodes them)
    return pick([c for body in K.SNAPPY_BODIES for c in K.snappy_cases(body)])


def _decode_call(codec, flags):
    def call(eng):
        N, L = _native()
        what = N.CODEC_LZ4_BLOCK if codec == "lz4" else N.CODEC_SNAPPY_RAW
        return lambda idx, i, o, l, out, oo, oc, r: eng.batch_device(what, N.OP_DECOMPRESS, flags, len(idx), i, o, l, out, oo, oc, r)
    return call


for _codec in ("lz4", "snappy"):
    @_list("%s-decode" % _codec, codec=_codec)
    def _blocks(codec):
        """run under every (flags, window) of capacity_cases.PATHS: the GPU test passes the flags"""
        return dict(cases=_block_cases(codec), call=lambda eng, flags=0: _decode_call(codec, flags)(eng))

    @_list("%s-decode-big" % _codec, codec=_codec)
    def _big(codec):
        """the ~100 KiB stream under CJ_FLAG_BIG_CHUNKS (the slab mode) among small chunks: the largest result straddles the line"""
        import capacity_cases as K
        from cramjam_amd import _native as N
        big, small = pick(K.big_cases(codec), 2), _block_cases(codec)[:8]                # (every big case is the same stream: the small ones are their decoys)
        cases = [big[k] for k in (1, 0, 2, 3, 4, 5, 6, 7)] + small                        # (the first, an accepted one, to place B)
        return dict(cases=cases, call=_decode_call(codec, N.FLAG_BIG_CHUNKS))



@_list("lz4-sizes")
def _lz4_sizes():
    """cj_batch_sizes_device over the blocks of tests/batch_sizes_cases.py with the oracle's size"""
    import batch_sizes_cases as S
    cs = pick([sized(dict(bytes=b, base=t), S.expected_size(b)) for t, b, _ in S.lz4_cases(big=False) if len(b) <= 80000])

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_batch_sizes_device(eng.h, N.CODEC_LZ4_BLOCK, 0, len(idx), i, o, l, r, None))
    return dict(cases=cs, call=call)


# ---- the encoders of tests/neighbour_cases.py: LZ4, Snappy, LZ4 with a dictionary, DEFLATE / zlib / gzip, Zstandard -------------------------------
def _encoder(codec):
    import neighbour_cases as NC
    cs = pick(NC.encoder_cases(codec))
    out = dict(cases=cs, encoder=True, refuses=False, call=lambda eng: lambda idx, *a: NC.encode_call(eng, codec, len(idx))(*a))
    if codec == "lz4_dict":
        import lz4_dict_model as D
        out["dictionary"] = D.dictionary(NC.DICT_LEN)
    if codec.startswith("deflate") or codec == "zstd":                                   # a capacity one byte short: the model's refusal
        if codec == "zstd":
            import zstd_enc_cases as E
            model = lambda raw, cap: E.model(raw, 0, cap)[:2]
        else:
            import deflate_enc_cases as E
            wrap = NC.ENCODERS.index(codec) - 3
            model = lambda raw, cap: E.model(raw, wrap, cap)[:2]
        for k in (5, 6, 7, 8):                                                            # one per place
            r, o = model(cs[k]["bytes"], cs[k]["result"] - 1)
            assert r < 0
            cs[k] = dict(cs[k], cap=cs[k]["result"] - 1, result=r, out=b"")
        out["refuses"] = True
    return out


for _codec in ("lz4", "snappy", "lz4_dict", "deflate_raw", "deflate_zlib", "deflate_gzip", "zstd"):
    LISTS["%s-encode" % _codec] = functools.partial(_encoder, _codec)


# ---- LZ4 blocks against a dictionary -------------------------------------------------------------------------------------------------------------
@_list("lz4_dict-decode")
def _dict_decode():
    import lz4_dict_model as D
    import neighbour_cases as NC

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r, d: N.check(L.cj_dict_batch_device(eng.h, N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, 0, len(idx), i, o, l, out, oo, oc, r, d, NC.DICT_LEN, None))
    return dict(cases=pick(NC.lz4_dict_cases()), call=call, dictionary=D.dictionary(NC.DICT_LEN))


@_list("lz4_dict-sizes")
def _dict_sizes():
    import lz4_dict_model as D
    import neighbour_cases as NC

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_dict_batch_sizes_device(eng.h, N.CODEC_LZ4_BLOCK, 0, len(idx), i, o, l, r, NC.DICT_LEN, None))
    return dict(cases=pick([sized(c, D.size_walk(c["bytes"], NC.DICT_LEN)) for c in NC.lz4_dict_cases()]), call=call)


# ---- DEFLATE / zlib / gzip, Zstandard, BGZF: decode and sizes ------------------------------------------------------------------------------------
def _deflate(wrap, sizes):
    import neighbour_cases as NC

    def call(eng):
        N, L = _native()
        if sizes:
            return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_sizes_device(eng.h, wrap, 0, len(idx), i, o, l, r, None))
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(eng.h, wrap, N.OP_DECOMPRESS, 0, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=pick(NC.deflate_size_cases(wrap) if sizes else NC.deflate_cases(wrap)), call=call)


for _wrap, _name in enumerate(("deflate_raw", "deflate_zlib", "deflate_gzip")):
    LISTS["%s-decode" % _name] = functools.partial(_deflate, _wrap, False)
    LISTS["%s-sizes" % _name] = functools.partial(_deflate, _wrap, True)


@_list("zstd-decode")
def _zstd_decode():
    import neighbour_cases as NC

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_device(eng.h, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=pick(NC.zstd_cases()), call=call)


@_list("zstd-sizes")
def _zstd_sizes():
    """the recorded cases of tests/zstd_cases.py whose size query is decided by the record: result = libzstd's verdict with room that
    never runs out"""
    import zstd_cases as Z
    cs = [c for c in Z.load_cases() if len(c.stream) <= 70000 and c.verdicts[1] != Z.E_OUT_TOO_SMALL and not (c.verdicts[1] < 0 and Z.size_query_may_miss(c.stream, c.verdicts[1]))]

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_sizes_device(eng.h, N.ZSTD_FRAMES, 0, len(idx), i, o, l, r, None))
    return dict(cases=pick([sized(dict(bytes=c.stream, base=c.name), c.verdicts[1]) for c in cs]), call=call)


def _bgzf(sizes):
    import neighbour_cases as NC

    def call(eng):
        N, L = _native()
        if sizes:
            return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_sizes_device(eng.h, 0, 0, len(idx), i, o, l, r, None))
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(eng.h, 0, N.OP_DECOMPRESS, 0, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=pick(NC.bgzf_size_cases() if sizes else NC.bgzf_decode_cases()), call=call)


LISTS["bgzf-decode"] = functools.partial(_bgzf, False)
LISTS["bgzf-sizes"] = functools.partial(_bgzf, True)


# ---- ORC streams: the golden streams of the four codecs, whole, one byte short of room, and cut --------------------------------------------------
ORC_BS = 65536


def _orc(codec, sizes):
    """the golden streams pyarrow wrote with 64 KiB blocks (tests/orc_model.py): accepted at their decoded length; refused by the
    model's rules with one byte less room (CJ_E_OUT_TOO_SMALL, nothing written) and, cut inside their last chunk, by the walk"""
    import orc_model as M
    gs = [g for g in M.golden_of(codec, ORC_BS) if 0 < g["decoded_len"] <= 200000]
    cs = []
    for g in gs:
        sizes_of = [c[3] for c in g["chunks"]]
        assert M.verdict(M.walk(g["stream"])[0], sizes_of, ORC_BS, g["decoded_len"]) == g["decoded_len"]
        cs.append(dict(bytes=g["stream"], cap=g["decoded_len"], result=g["decoded_len"], out=None, sha=g["sha256"], written=0, base=g["name"], size=g["decoded_len"]))
    short = [dict(c, cap=c["cap"] - 1, result=M.verdict(0, [c["cap"]], 1 << 30, c["cap"] - 1), out=b"") for c in cs[:2]]
    cut = [dict(c, bytes=c["bytes"][:-1], result=M.walk(c["bytes"][:-1])[0], out=b"") for c in cs[:2]]
    for c in cut:
        c["size"] = c["result"]
    assert all(c["result"] < 0 for c in short + cut)
    cs = pick(cs, PER_PLACE - 1) + short + cut
    if sizes:
        cs = [sized(c, c["size"]) for c in cs]

    def call(eng):
        N, L = _native()
        kind = M.KINDS[codec]
        if sizes:
            return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_orc_sizes_device(eng.h, kind, 0, ORC_BS, len(idx), i, o, l, r, None))
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_orc_batch_device(eng.h, kind, N.OP_DECOMPRESS, 0, ORC_BS, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=cs, call=call)


for _codec in ("zlib", "snappy", "lz4", "zstd"):
    LISTS["orc_%s-decode" % _codec] = functools.partial(_orc, _codec, False)
    LISTS["orc_%s-sizes" % _codec] = functools.partial(_orc, _codec, True)


# ---- Parquet column chunks: the small golden chunks of the five codecs ---------------------------------------------------------------------------
def _parquet_chunks(codec):
    import parquet_model as M
    gs = [g for g in M.golden_of(codec, big=False) if 0 < g["decoded_len"] <= 200000]
    cs = []
    for g in gs:
        assert M.verdict(g["chunk"], codec, g["decoded_len"], verify_crc=True) == M.verdict(g["chunk"], codec) == g["decoded_len"]
        cs.append(dict(bytes=g["chunk"], cap=g["decoded_len"], result=g["decoded_len"], out=None, sha=g["sha256"], written=0, base=g["name"], pages=g["pages"]))
    short = [dict(c, cap=c["cap"] - 1, result=M.verdict(c["bytes"], codec, c["cap"] - 1), out=b"") for c in cs[:2]]
    cut = [dict(c, bytes=c["bytes"][:-1], result=M.verdict(c["bytes"][:-1], codec, c["cap"]), out=b"", pages=None) for c in cs[:2]]
    assert all(c["result"] < 0 for c in short + cut)
    return pick(cs, PER_PLACE - 1) + short + cut


def _parquet(codec, mode):
    """mode: "decode", "decode-crc" (PARQUET_FLAG_VERIFY_CRC), "sizes"; the model's rules give the refusals: one byte less room
    (CJ_E_OUT_TOO_SMALL), a chunk cut inside its last page (CJ_E_PARQUET_HEADER)"""
    import parquet_model as M
    cs = _parquet_chunks(codec)
    if mode == "sizes":
        cs = [sized(c, M.verdict(c["bytes"], codec)) for c in cs]

    def call(eng):
        N, L = _native()
        what = M.CODECS[codec]
        if mode == "sizes":
            return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_parquet_sizes_device(eng.h, what, 0, len(idx), i, o, l, r, None))
        flags = N.PARQUET_FLAG_VERIFY_CRC if mode == "decode-crc" else 0
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_parquet_batch_device(eng.h, what, N.OP_DECOMPRESS, flags, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=cs, call=call)


for _codec in ("uncompressed", "snappy", "gzip", "zstd", "lz4_raw"):
    for _mode in ("decode", "decode-crc", "sizes"):
        LISTS["parquet_%s-%s" % (_codec, _mode)] = functools.partial(_parquet, _codec, _mode)


@_list("parquet-pages")
def _parquet_pages():
    """cj_parquet_pages_device over far chunks: the result is the page count; the rows land in a table of the call's own (row offsets
    count rows, not bytes) and every word — `payload` and `out_at` among them, both relative to the chunk — is the golden table's"""
    import parquet_model as M
    cs = [c for codec in ("snappy", "gzip") for c in _parquet_chunks(codec)]
    cs = [sized(c, len(c["pages"]) if c["pages"] is not None else M.HEADER) for c in cs if c["result"] >= 0 or c["pages"] is None]

    def call(eng):
        import device_batch as DB
        N, L = _native()

        def run(idx, i, o, l, out, oo, oc, r):
            counts = [max(cs[k]["result"], 0) for k in idx]
            ooff, total = DB.out_slots(np.array(counts, np.uint64) * 64)
            b = DB._Batch(eng, len(idx))
            try:
                tab = b.buffer(total, DB.FILL)
                row_off, row_cap = b.rows(ooff // 64, counts)
                N.check(L.cj_parquet_pages_device(eng.h, 0, len(idx), i, o, l, tab, row_off, row_cap, r, None))
                eng.sync()
                got = eng.d2h(tab, total)
            finally:
                b.free()
            keep = DB.untouched(ooff, np.array(counts, np.int64) * 64, total)
            assert (got[keep] == DB.FILL).all(), "a byte outside the tables changed"
            for k, at, n in zip(idx, ooff, counts):
                if n:
                    assert got[int(at):int(at) + 64 * n].view(np.int64).reshape(-1, 8).tolist() == cs[k]["pages"], ("page table", k)
        return run
    return dict(cases=cs, call=call)


# ---- Blosc chunks ------------------------------------------------------------------------------------------------------------------------------------
def _blosc_decode(which):
    import neighbour_cases as NC
    flags, cs = NC.blosc_cases(which)

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_blosc_batch_device(eng.h, N.OP_DECOMPRESS, i, o, l, out, oo, oc, r, len(idx), None, flags, None))
    return dict(cases=pick(cs), call=call, flags=flags)


LISTS["blosc_blosclz-decode"] = functools.partial(_blosc_decode, "blosclz")
LISTS["blosc_zcodecs-decode"] = functools.partial(_blosc_decode, "zcodecs")


@_list("blosc-sizes")
def _blosc_sizes():
    """cj_blosc_chunk_sizes_device over the LZ4 fixtures of tests/blosc_cases.py: nbytes of the valid chunks, the model's class for the
    malformed ones whose HEADER is refused (the query reads the header and the block starts)"""
    import blosc_cases as B
    import blosc_model as BM
    cs = [sized(dict(bytes=v["bytes"], base=v["name"]), v["nbytes"]) for v in B.valid() if len(v["bytes"]) <= 80000]
    refused = [sized(dict(bytes=v["bytes"], base=v["name"]), BM.CODE[BM.UNSUPPORTED]) for v in B.valid(supported=False) if len(v["bytes"]) <= 80000]
    cs = pick(cs, PER_PLACE - 1) + refused[:4]

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_blosc_chunk_sizes_device(eng.h, 0, len(idx), i, o, l, r, None))
    return dict(cases=cs, call=call)


# ---- LZ4 frames and framed Snappy streams: the oracle decides (tests/test_frames_gpu.py holds the library to it, refusals included) --------------
FRAME_SIZES = (0, 1, 100, 8192, 65535, 65536, 65537)


@functools.lru_cache(maxsize=None)
def _frames(fmt):
    """the frames of tests/test_frame_batch_gpu.py that need no GPU to build — the golden vectors and files, the oracle's frames of
    every block size and flag, a skippable frame, a frame behind it, by-hand chunk sequences — and that file's mutants of each"""
    import base64
    import json
    import os
    import random
    import struct

    import oracle
    import test_frame_batch_gpu as T
    from framing import SNAPPY_IDENT, snappy_chunk, snappy_compressed, snappy_stored
    good = []
    if fmt == "lz4":
        g = json.load(open(os.path.join(T.GOLDEN, "golden_frames.json")))
        good += [base64.b64decode(v["frame"]) for v in g["vectors"]]
        for i, n in enumerate(FRAME_SIZES):
            d = T._text(n, i) if i % 2 else T._rand(n, i)
            for bs, fl in ((4, 0), (5, oracle.LZ4F_LINKED), (6, oracle.LZ4F_BLOCK_CHECKSUM | oracle.LZ4F_CONTENT_SIZE), (7, oracle.LZ4F_NO_CONTENT_CHECKSUM)):
                good.append(oracle.lz4_frame_compress(d, bs, fl)[1])
        good.append(struct.pack("<II", 0x184D2A53, 5) + b"skip!")
        good.append(good[-1] + good[0])
        good.append(open(os.path.join(T.GOLDEN, "plaintext.txt.lz4"), "rb").read())
        bound, mutants = oracle.lz4_frame_decompress_bound, T._lz4_mutants
    else:
        for i, n in enumerate(FRAME_SIZES):
            good.append(oracle.snappy_frame_compress(T._text(n, 100 + i) if i % 2 else T._rand(n, 100 + i))[1])
        p1, p2 = T._text(3000, 1), T._text(70000, 2)[:65536]
        good.append(SNAPPY_IDENT + snappy_chunk(0xfe, b"\0" * 7) + snappy_stored(p1) + snappy_chunk(0x80, b"xyz") + SNAPPY_IDENT
                    + snappy_compressed(p2, oracle.snappy_compress(p2)[1]) + snappy_stored(b""))
        good.append(SNAPPY_IDENT + SNAPPY_IDENT + snappy_stored(T._rand(65536, 3)))
        good.append(open(os.path.join(T.GOLDEN, "plaintext.txt.snappy"), "rb").read())
        bound, mutants = oracle.snappy_frame_decompress_len, T._snappy_mutants
    good = [f for f in good if len(f) <= 200000 and bound(f) <= 200000]
    rnd, out = random.Random(1234), []
    for f in good:
        cap = max(bound(f), 0)
        out.append((f, cap))
        out += [(m, cap) for m in mutants(f, rnd)]
        if cap > 0:
            out.append((f, cap - 1))
    return out


def _frame_list(fmt, mode):
    import oracle
    dec = oracle.lz4_frame_decompress if fmt == "lz4" else oracle.snappy_frame_decompress
    size = oracle.lz4_frame_decompress_bound if fmt == "lz4" else oracle.snappy_frame_decompress_len
    cs, frames = [], _frames(fmt)
    if mode == "sizes" and fmt == "lz4":
        # the intact frames under the damages of tests/batch_sizes_child.py, where the suite holds the library's bound to the oracle's.  (Not
        # test_frame_batch_gpu's cuts: for a frame cut inside its end mark or content checksum the library's bound — host function and
        # device alike — is CJ_E_LZ4F_INCOMPLETE, the oracle's the blocks' sum; no test pins either.)
        whole = [f for f, cap in frames if len(f) >= 16 and f[:4] == b"\x04\x22\x4d\x18" and dec(f, cap)[0] >= 0 and (f, cap - 1) in frames]
        frames = [(g, 0) for f in whole for g in (f, f[:len(f) // 2], f[:6], f[:9], b"\x05" + f[1:], f[:4] + b"\xe4" + f[5:], f + b"trailing")]
    for f, cap in frames:
        if mode == "sizes":
            cs.append(sized(dict(bytes=f), size(f)))
        else:
            r, o = dec(f, cap)
            cs.append(dict(bytes=f, cap=cap, result=int(r), out=o if r >= 0 else b""))

    def call(eng):
        N, L = _native()
        what = N.FORMAT_LZ4_FRAME if fmt == "lz4" else N.FORMAT_SNAPPY_FRAMED
        if mode == "sizes":
            return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_frame_batch_sizes_device(eng.h, what, 0, len(idx), i, o, l, r, None))
        return lambda idx, i, o, l, out, oo, oc, r: eng.frame_batch_device(what, N.OP_DECOMPRESS, 0, len(idx), i, o, l, out, oo, oc, r)
    return dict(cases=pick(cs), call=call)


def _piece_models(codec):
    """raw piece -> the stream the codec's plain encoder writes for it: the C models of tests/hostsim (tests/neighbour_cases.py)"""
    if codec in ("lz4", "snappy"):
        from test_enc2_model import model_lib, model_lz4, model_snappy
        L = model_lib()
        return (lambda p: model_lz4(L, p)) if codec == "lz4" else (lambda p: model_snappy(L, p))
    if codec == "zstd":
        import zstd_enc_cases as E
        return lambda p: E.model(p, 0)[1]
    import deflate_enc_cases as E
    return lambda p: E.model(p, 0)[1]                                                    # raw DEFLATE


def _encoder_inputs(n=32):
    """inputs of tests/neighbour_cases.py at a fixed stride, and two of its longest joined: more than one piece"""
    import neighbour_cases as NC
    ins = [c["bytes"] for c in NC.encoder_inputs()]
    step = ins[::max(1, len(ins) // n)][:n]
    long = [c for c in ins if len(c) == 65536]
    return step + [long[0] + long[-1], long[-1] + long[1][:4097]]


def _with_refusals(cs, code, short):
    """four of the cases (one per place) at a capacity `short(case)` that the entry refuses with `code`, writing nothing"""
    for k in (4, 5, 6, 7):
        cs[k] = dict(cs[k], cap=short(cs[k]), result=code, out=b"", written=0)
    return cs


def _frame_encode(fmt):
    """the single-call layouts (include/cramjam_hip.h, cj_frame_batch_device) around the block models' payloads of each 64 KiB piece"""
    import struct

    import oracle
    from framing import SNAPPY_IDENT, snappy_compressed, snappy_stored
    N, L = _native()
    model = _piece_models(fmt)
    cs = []
    for d in _encoder_inputs():
        pieces = [d[k:k + 65536] for k in range(0, len(d), 65536)]
        if fmt == "lz4":
            f = b"\x04\x22\x4d\x18\x64\x40" + bytes([(oracle.xxh32(b"\x64\x40") >> 8) & 0xFF])
            for p in pieces:
                c = model(p)
                f += struct.pack("<I", len(p) | 0x80000000) + p if len(c) >= len(p) else struct.pack("<I", len(c)) + c
            f += struct.pack("<II", 0, oracle.xxh32(d))
            cap = L.cj_lz4_frame_compress_bound(len(d))
        else:
            f = SNAPPY_IDENT
            for p in pieces:
                c = model(p)
                f += snappy_stored(p) if len(c) >= len(p) - len(p) // 8 else snappy_compressed(p, c)
            cap = L.cj_snappy_frame_max_compress_len(len(d))
        assert (oracle.lz4_frame_decompress if fmt == "lz4" else oracle.snappy_frame_decompress)(f, len(d)) == (len(d), d) and len(f) <= cap
        cs.append(dict(bytes=d, cap=cap, result=len(f), out=f))

    def call(eng):
        what = N.FORMAT_LZ4_FRAME if fmt == "lz4" else N.FORMAT_SNAPPY_FRAMED
        return lambda idx, i, o, l, out, oo, oc, r: eng.frame_batch_device(what, N.OP_COMPRESS, 0, len(idx), i, o, l, out, oo, oc, r)
    return dict(cases=_with_refusals(cs, -14, lambda c: c["result"] - 1), call=call, encoder=True)      # CJ_E_FRAME_WRITE


for _fmt in ("lz4", "snappy"):
    LISTS["%s_frames-decode" % _fmt] = functools.partial(_frame_list, _fmt, "decode")
    LISTS["%s_frames-sizes" % _fmt] = functools.partial(_frame_list, _fmt, "sizes")
    LISTS["%s_frames-encode" % _fmt] = functools.partial(_frame_encode, _fmt)


# ---- the container encoders: BGZF and ORC byte for byte as include/cramjam_hip.h lays them out around the plain encoders' streams; Blosc read back ----
@_list("bgzf-encode")
def _bgzf_encode():
    """members of 65 280 input bytes: the 18-byte header, the raw DEFLATE model's block, CRC-32 and ISIZE; then the marker"""
    import struct
    import zlib

    import bgzf_model as B
    model = _piece_models("deflate_raw")
    cs = []
    for d in _encoder_inputs():
        s = b""
        for k in range(0, len(d), B.PIECE):
            p = d[k:k + B.PIECE]
            c = model(p)
            s += B.MARKER[:16] + struct.pack("<H", 18 + len(c) + 8 - 1) + c + struct.pack("<II", zlib.crc32(p), len(p))
        s += B.MARKER
        assert B.decode(s, len(d)) == (len(d), d) and len(s) <= B.compress_bound(len(d))
        cs.append(dict(bytes=d, cap=B.compress_bound(len(d)), result=len(s), out=s))

    def call(eng):
        N, L = _native()
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(eng.h, 0, N.OP_COMPRESS, 0, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=_with_refusals(cs, -6, lambda c: c["result"] - 1), call=call, encoder=True)       # CJ_E_OUT_TOO_SMALL: the stream does not fit


def _orc_encode(codec):
    """pieces of 64 KiB: the plain encoder's stream where it is shorter than the piece, else the piece as an original chunk"""
    import orc_model as M
    model = _piece_models({"zlib": "deflate_raw"}.get(codec, codec))
    cs = []
    for d in _encoder_inputs():
        chunks = []
        for k in range(0, len(d), ORC_BS):
            p = d[k:k + ORC_BS]
            c = model(p)
            chunks.append((0, c) if len(c) < len(p) else (1, p))
        s = M.frame(chunks)
        M.check_encoded(s, d, ORC_BS, codec)
        cs.append(dict(bytes=d, cap=M.compress_bound(len(d), ORC_BS), result=len(s), out=s))

    def call(eng):
        N, L = _native()
        kind = M.KINDS[codec]
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_orc_batch_device(eng.h, kind, N.OP_COMPRESS, 0, ORC_BS, len(idx), i, o, l, out, oo, oc, r, None))
    return dict(cases=_with_refusals(cs, M.OUT_TOO_SMALL, lambda c: c["cap"] - 1), call=call, encoder=True)      # (a capacity below the bound)


for _codec in ("zlib", "snappy", "lz4", "zstd"):
    LISTS["orc_%s-encode" % _codec] = functools.partial(_orc_encode, _codec)


@_list("blosc-encode")
def _blosc_encode():
    """the inputs of the valid fixtures of tests/blosc_cases.py (typesize 4, shuffle, LZ4, clevel 5).  No model writes this encoder's
    bytes: as in tests/test_blosc_gpu.py the chunk is read back by tests/blosc_model.py — its header's fields, its decoded bytes"""
    import ctypes as C

    import blosc_cases as B
    import blosc_model as BM
    raws, seen = [], set()
    for v in B.valid():
        r = v["recipe"]
        if (r["kind"], r["size"], r["seed"]) not in seen and 0 < r["size"] <= 70000 and r["size"] % 4 == 0:
            seen.add((r["kind"], r["size"], r["seed"]))
            raws.append(B.raw_of(v))

    def verify(raw):
        def check(chunk):
            h, _ = BM.parse(chunk)
            assert h["typesize"] == 4 and h["nbytes"] == len(raw) and BM.decode(chunk, len(raw)) == raw, ("the chunk does not read back", len(raw))
        return check
    cs = [dict(bytes=r, cap=len(r) + 32, result=None, at_least=16, verify=verify(r), out=None) for r in raws]
    cs = pick(cs)
    for k in (4, 5):                                                                     # fewer bytes than a header: CJ_E_COMPRESS_FAILED
        cs[k] = dict(cs[k], cap=15, result=-2, verify=None)

    def call(eng):
        N, L = _native()
        params = N.BloscParams(4, 1, 5, 1, 0)
        return lambda idx, i, o, l, out, oo, oc, r: N.check(L.cj_blosc_batch_device(eng.h, N.OP_COMPRESS, i, o, l, out, oo, oc, r, len(idx), C.byref(params), 0, None))
    return dict(cases=cs, call=call, encoder=True)
