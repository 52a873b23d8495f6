"""No batch result depends on what the engine's scratch held.  cj_engine reuses some twenty device buffers and a few
pinned ones call after call; in production every call finds them full of an earlier batch's records, verdicts, counters, done flags and
slot contents.  The rule: every word a kernel or the host reads from them was written earlier in the same call.  Here every family of
batches that reaches one of those buffers runs once on a fresh engine (the single-buffer API: once on the default engine) and then under
four preparations:

  zeros    cj_debug_scratch_fill pattern 0: 0x00 in every byte of every buffer that is not a state carrier
  ones     pattern 1: 0xFF
  hash     pattern 2 + SEED: a hash of (word index, pattern) in every 32-bit word
  residue  no fill: a larger batch of the same family first (the full case list, then its first 130 cases — neither a multiple of 64 nor
           of any grid, so verdicts, lists and slots of chunks >= 130 lie stale behind the live ones); a list of 130 cases or fewer
           runs reversed first, then in order

After each fill the first and last 64 bytes of every filled buffer are read back (cj_debug_scratch_peek) and held to the pattern.
The case lists and harnesses are the suite's own, by import (capacity_cases + its run_and_check on tests/device_batch.py, neighbour_cases +
its device / host_check, the generators of test_large_gpu / test_frames_gpu / test_frame_batch_gpu): the expected
values are the CPU oracle's, the models' or recorded reference verdicts, never an earlier GPU run's, and the harnesses' assertions —
64 guard bytes of 0xA5 around every output slot, nothing written behind a result, the input read back unchanged — hold under every
preparation.  On top of them all runs of one family must give identical results and identical bytes.

The wave-per-chunk and lane-per-chunk block decoders use no scratch and are left out.  h_res is the one buffer no family reaches: only a
sliced host batch of >= 512 chunks and >= 128 MiB fills it (csrc/engine.hip: batch_host_sliced), too large for this file; the audit of
DESIGN.md 5.10b covers it by reading.  h_count carries state between calls by design and is never filled."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import capacity_cases as K
import neighbour_cases as NC
import oracle
import test_frame_batch_gpu as TFB
import test_frames_gpu as TF
import test_large_gpu as TL
from cramjam_amd import _native as N

pytestmark = pytest.mark.gpu
LZ4, SN, DEC, ENC = N.CODEC_LZ4_BLOCK, N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS, N.OP_COMPRESS
SEED = 0x5EED
PATTERN = {"zeros": 0, "ones": 1, "hash": 2 + SEED}
PREPS = ("zeros", "ones", "hash", "residue")
HEAD = 130
RING = "zero"                                      # the neighbour harness's control ring: what lies around the INPUT is not this file's subject
NEVER_REACHED = {"h_res"}                          # (the reason: this file's head)
DEFAULT_ENGINE_ONLY = {"d_frame", "d_big", "d_bigtab"}      # what only the single-buffer API reaches: it runs on the default engine


# ---- the exports ---------------------------------------------------------------------------------------------------------------------------
def _names():
    L = N.lib()
    return [L.cj_debug_scratch_name(i).decode() for i in range(L.cj_debug_scratch_count())]


def _carriers():
    L = N.lib()
    return {n for i, n in enumerate(_names()) if L.cj_debug_scratch_carries_state(i) == 1}


def fill_words(w0, n, pattern):
    """words [w0, w0 + n) of a buffer filled with `pattern` >= 2: fill_word of csrc/engine.hip, restated"""
    m32 = np.uint64(0xFFFFFFFF)
    w = np.arange(w0, w0 + n, dtype=np.uint64)
    h = ((w & m32) * np.uint64(0x9E3779B1) & m32) ^ ((w >> np.uint64(32)) * np.uint64(0x85EBCA77) & m32) ^ np.uint64(pattern * 0xC2B2AE3D & 0xFFFFFFFF)
    h ^= h >> np.uint64(15); h = h * np.uint64(0x2C1B3C6D) & m32
    h ^= h >> np.uint64(12); h = h * np.uint64(0x297A2D39) & m32
    h ^= h >> np.uint64(15)
    return h.astype("<u4")


def expected_fill(pattern, off, n):
    if pattern < 2:
        return bytes([0xFF if pattern else 0x00]) * n
    w0 = off // 4
    return fill_words(w0, (off + n + 3) // 4 - w0, pattern).tobytes()[off - 4 * w0:off - 4 * w0 + n]


def test_the_hash_pattern_is_no_constant():
    a = fill_words(0, 4096, PATTERN["hash"])
    assert len(set(a.tolist())) >= 4090 and (fill_words(1 << 32, 4, 2) != fill_words(0, 4, 2)).all() and (fill_words(0, 64, 2) != fill_words(0, 64, 3)).all()
    assert expected_fill(7, 5, 9) == fill_words(1, 3, 7).tobytes()[1:10]


def _fill_and_peek(h, pattern):
    """fill every scratch buffer of engine h (None: the default engine) and prove that the fill landed; returns {name: bytes filled}"""
    L = N.lib()
    names = _names()
    filled = (C.c_uint64 * len(names))()
    N.check(L.cj_debug_scratch_fill(h, pattern, filled))
    buf = C.create_string_buffer(64)
    for i, (name, cap) in enumerate(zip(names, filled)):
        if cap == 0:
            continue
        assert name not in _carriers(), name
        for off in sorted({0, max(cap - 64, 0)}):
            n = min(64, cap - off)
            N.check(L.cj_debug_scratch_peek(h, i, off, buf, n))
            assert buf.raw[:n] == expected_fill(pattern, off, n), ("the fill did not land", name, pattern, off, cap)
    return dict(zip(names, filled))


# ---- one run of a batch: the suite's harness around it, then what it computed as a list of (result, crc of the bytes) per chunk -------------
def _sig(res, out, ooff, cases):
    crc = lambda i, r: zlib.crc32(out[int(ooff[i]):int(ooff[i]) + r].tobytes())
    return [(int(r), crc(i, int(r)) if r > 0 and not c.get("sized") else None) for i, (r, c) in enumerate(zip(res, cases))]


def capacity_run(codec, flags):
    """capacity_cases.run_and_check: the oracle's result and bytes, both guards, nothing behind an accepted result"""
    def run(e, key, cases):
        return _sig(*K.run_and_check(e, codec, flags, key, cases), cases)
    return run


def device_run(call_of, dictionary=None):
    """neighbour_cases.device: the same, and the input read back unchanged.  call_of(e, n) -> the call over n chunks"""
    def run(e, key, cases):
        return _sig(*NC.device(e, key, cases, RING, call_of(e, len(cases)), dictionary=dictionary), cases)
    return run


def host_run(call):
    """a host entry (the library's own staging: d_in, d_out, d_meta, h_in, h_out, the host rows) held by neighbour_cases.host_check.
    call(e, cases) -> (results, outputs)"""
    def run(e, key, cases):
        res, outs = call(e, cases)
        NC.host_check(key, cases, res, outs)
        return [(int(r), zlib.crc32(bytes(o)) if r > 0 else None) for r, o in zip(res, outs)]
    return run


def _raws(cs): return [c["bytes"] for c in cs]
def _caps(cs): return [c["cap"] for c in cs]


# ---- the families: name -> () -> (default_engine, [(key, cases, run)]) -----------------------------------------------------------------------
FAMILIES = {}


def family(name, default_engine=False):
    def add(make):
        FAMILIES[name] = (default_engine, make)
        return make
    return add


# d_pmeta, d_lanelist, d_tab, d_sync: the workgroup decoder behind the parse kernel and with the parse inside it, on every window
LDS_PATHS = [p for p in K.PATHS if p.id not in ("wave-per-chunk", "lane-per-chunk")]
assert [p.id for p in LDS_PATHS] == ["lds+parse-kernel", "lds+fused-parse", "default", "le32k", "le32k+parse-kernel", "le32k+fused-parse", "le16k",
                                     "le16k+parse-kernel", "le16k+fused-parse"]
for _p in LDS_PATHS:
    for _codec, _cname in ((LZ4, "lz4"), (SN, "snappy")):
        family("%s-%s" % (_cname, _p.id))(lambda c=_codec, n=_cname, f=_p.values[0]: [
            ((n, "b"), K.lz4_cases("b") if c == LZ4 else K.snappy_cases("b"), capacity_run(c, f))])


def _above(codec):
    cs = K.lz4_cases("b") if codec == LZ4 else K.snappy_cases("b")
    n = 16384 + 41                                 # above CJ_FUSED_MAX_CHUNKS: the engine picks the parse kernel itself
    assert len(cs) < n
    return [(("above", codec), [cs[i % len(cs)] for i in range(n)], capacity_run(codec, 0))]


family("lz4-default-above-the-one-kernel-limit")(lambda: _above(LZ4))
family("snappy-default-above-the-one-kernel-limit")(lambda: _above(SN))
# d_biglist, d_bigrecs, d_bigmisc, d_bigslabtab
family("lz4-big-chunks")(lambda: [(("big", LZ4), K.big_cases("lz4"), capacity_run(LZ4, N.FLAG_BIG_CHUNKS))])
family("snappy-big-chunks")(lambda: [(("big", SN), K.big_cases("snappy"), capacity_run(SN, N.FLAG_BIG_CHUNKS))])


# d_big, d_bigtab, d_in, d_out, d_frame, h_in, h_out: the single-buffer API, on the default engine
def _single_items():
    import cramjam_amd as cramjam
    L = N.lib()
    # test_large_gpu's many-slab recipe at five pieces: 777 zeros, then synth-v1 pieces — chunk boundaries off the slab grid, ~330 KiB
    many = bytes(777) + b"".join(oracle.synth_v1(TL.PIECE, i) for i in range(5))
    text = dict(TL.CASES)["text-random-text"]      # ~230 KiB: text, two incompressible pieces, text
    mixed = TF.mixed_data(5, 20, 30000, 20000)
    lz, sn = oracle.lz4_compress_raw(many)[1], oracle.snappy_compress(many)[1]
    assert len(lz) > 8192 and len(many) > 4 * TL.PIECE and len(text) > 3 * TL.PIECE

    def linked(data):
        cap = L.cj_lz4_frame_compress_bound(len(data))
        buf = C.create_string_buffer(cap)
        r = L.cj_lz4_frame_compress_linked(data, len(data), C.cast(buf, C.c_void_p), cap, 0)
        assert r > 0
        return buf.raw[:r]

    def frame_ok(frame, data):
        assert oracle.lz4_frame_decompress(frame) == (len(data), data)
        return frame

    def snappy_ok(stream, data):
        assert oracle.snappy_frame_decompress(stream) == (len(data), data)
        return stream

    def is_(got, want):
        assert got == want
        return got

    items = [("lz4-decode-many-slabs", lambda: is_(bytes(cramjam.lz4.decompress_block(lz, output_len=len(many))), many)),
             ("snappy-decode-many-slabs", lambda: is_(bytes(cramjam.snappy.decompress_raw(sn)), many)),
             ("lz4-decode-text", lambda: is_(bytes(cramjam.lz4.decompress_block(oracle.lz4_compress_raw(text)[1], output_len=len(text))), text)),
             ("lz4-encode", lambda: (lambda b: is_(oracle.lz4_decompress_raw(b, len(text)), (len(text), text)) and b)(bytes(cramjam.lz4.compress_block(text, store_size=False)))),
             ("snappy-encode", lambda: (lambda b: is_(oracle.snappy_decompress(b), (len(text), text)) and b)(bytes(cramjam.snappy.compress_raw(text)))),
             ("lz4-encode-10000", lambda: (lambda b: is_(oracle.lz4_decompress_raw(b, 10000), (10000, text[:10000])) and b)(bytes(cramjam.lz4.compress_block(text[:10000], store_size=False)))),
             ("lz4-frame-encode", lambda: frame_ok(TF.lz4f_compress(mixed)[1], mixed)),
             ("lz4-frame-encode-linked", lambda: frame_ok(linked(mixed), mixed)),
             ("lz4-frame-decode", lambda: is_(TF.lz4f_decompress(oracle.lz4_frame_compress(mixed, 4, 0)[1]), (len(mixed), mixed))[1]),
             ("lz4-frame-decode-linked", lambda: is_(TF.lz4f_decompress(oracle.lz4_frame_compress(mixed, 4, oracle.LZ4F_LINKED)[1]), (len(mixed), mixed))[1]),
             ("lz4-frame-decode-large-blocks", lambda: is_(TF.lz4f_decompress(oracle.lz4_frame_compress(many, 7, 0)[1]), (len(many), many))[1]),
             ("snappy-framed-encode", lambda: snappy_ok(TF.abi_compress(mixed)[1], mixed)),
             ("snappy-framed-decode", lambda: is_(TF.abi_decompress(oracle.snappy_frame_compress(mixed)[1]), (len(mixed), mixed))[1])]

    def run(e, key, cases):
        assert e is None
        return [(name, zlib.crc32(bytes(fn()))) for name, fn in cases]
    return [("single", items, run)]


family("single-buffer-api", default_engine=True)(_single_items)


# d_fb, h_fb: frame batches, Blosc chunks, BGZF streams
def _frame_batch(fmt):
    L = N.lib()
    frames = TFB._lz4_frames() if fmt == N.FORMAT_LZ4_FRAME else TFB._snappy_streams()
    want = [oracle.lz4_frame_decompress(f) if fmt == N.FORMAT_LZ4_FRAME else oracle.snappy_frame_decompress(f) for f in frames]
    bound = L.cj_lz4_frame_decompress_bound if fmt == N.FORMAT_LZ4_FRAME else L.cj_snappy_frame_decompress_len
    cases = [dict(base="frame%d" % i, k=len(f), bytes=f, cap=max(bound(f, len(f)), 0) if f else 0, result=r, out=o, sha=None) for i, (f, (r, o)) in enumerate(zip(frames, want))]
    assert min(c["result"] for c in cases) >= 0
    raws = [c["out"] for c in cases if c["out"]]
    cbound = L.cj_lz4_frame_compress_bound if fmt == N.FORMAT_LZ4_FRAME else L.cj_snappy_frame_max_compress_len
    decode = oracle.lz4_frame_decompress if fmt == N.FORMAT_LZ4_FRAME else oracle.snappy_frame_decompress

    def compress(e, key, cs):                      # the frames the batch writes decode, by the oracle, to their inputs
        res, outs = e.batch_host(fmt, ENC, 0, cs, [cbound(len(r)) for r in cs], N.FRAMES)
        for r, o, raw in zip(res, outs, cs):
            assert r == len(o) > 0 and decode(bytes(o)) == (len(raw), raw)
        return [(int(r), zlib.crc32(bytes(o))) for r, o in zip(res, outs)]
    return [(("frames", fmt), cases, host_run(lambda e, cs: e.batch_host(fmt, DEC, 0, _raws(cs), _caps(cs), N.FRAMES))),
            (("frames-enc", fmt), raws, compress)]


family("lz4-frame-batch")(lambda: _frame_batch(N.FORMAT_LZ4_FRAME))
family("snappy-framed-batch")(lambda: _frame_batch(N.FORMAT_SNAPPY_FRAMED))


def _blosc(which):
    """d_fb / h_fb; the zcodecs also d_zstd_slots (Zstandard streams inside the chunks)"""
    L = N.lib()
    flags, cs = NC.blosc_cases(which)
    call_of = lambda e, n: lambda i, o, l, out, oo, oc, r: N.check(L.cj_blosc_batch_device(e.h, 0, i, o, l, out, oo, oc, r, n, None, flags, None))
    # (the host entry takes each chunk's capacity from its own header: the cases whose capacity is that — the neighbour sweep's choice)
    hs = NC.shuffled([c for c in cs if len(c["bytes"]) >= 16 and int.from_bytes(c["bytes"][4:8], "little") == c["cap"]])
    return [(("blosc", which), cs, device_run(call_of)),
            (("blosc", which, "host"), hs, host_run(lambda e, x: e.batch_host(0, DEC, flags, _raws(x), _caps(x), N.BLOSC, params=b"")))]


family("blosc-blosclz")(lambda: _blosc("blosclz"))
family("blosc-zcodecs")(lambda: _blosc("zcodecs"))


@family("bgzf")
def _bgzf():
    L = N.lib()
    cs, sz = NC.bgzf_decode_cases(), NC.bgzf_size_cases()
    dec = lambda e, n: lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(e.h, 0, DEC, 0, n, i, o, l, out, oo, oc, r, None))
    size = lambda e, n: lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_sizes_device(e.h, 0, 0, n, i, o, l, r, None))
    return [("bgzf", cs, device_run(dec)), ("bgzf-size", sz, device_run(size)),
            (("bgzf", "host"), NC.shuffled(cs), host_run(lambda e, x: e.batch_host(0, DEC, 0, _raws(x), _caps(x), N.BGZF)))]


# d_dict_stage, d_dict: the shared dictionary, both directions, at the device and the host entry
@family("lz4-dictionary")
def _dict():
    import lz4_dict_model as D
    L = N.lib()
    d = D.dictionary(NC.DICT_LEN)
    cs, en = NC.lz4_dict_cases(), NC.encoder_cases("lz4_dict")
    call = lambda op: lambda e, n: lambda i, o, l, out, oo, oc, r, dd: N.check(L.cj_dict_batch_device(e.h, LZ4, op, 0, n, i, o, l, out, oo, oc, r, dd, NC.DICT_LEN, None))
    host = lambda op: host_run(lambda e, x: e.batch_host(LZ4, op, 0, _raws(x), _caps(x), N.DICT, dictionary=d))
    return [("lz4-dict", cs, device_run(call(DEC), d)), (("lz4-dict", "host"), NC.shuffled(cs), host(DEC)),
            (("enc", "lz4_dict"), en, device_run(call(ENC), d)), (("enc", "lz4_dict", "host"), NC.shuffled(en), host(ENC))]


# d_deflate_slots (the DEFLATE encoder, BGZF compress), d_zstd_enc_slots, and the LZ4 / Snappy block encoders (no scratch of their own: the staging)
def _encoder(codec, kind, what, flags=0):
    cs = NC.encoder_cases(codec)
    return [(("enc", codec), cs, device_run(lambda e, n: NC.encode_call(e, codec, n))),
            (("enc", codec, "host"), NC.shuffled(cs), host_run(lambda e, x: e.batch_host(what, ENC, flags, _raws(x), _caps(x), kind)))]


for _w, _codec in enumerate(("deflate_raw", "deflate_zlib", "deflate_gzip")):
    family("encode-" + _codec)(lambda c=_codec, w=_w: _encoder(c, N.DEFLATE_COMPRESS, w))
family("encode-zstd")(lambda: _encoder("zstd", N.ZSTD_COMPRESS, N.ZSTD_FRAMES))
family("encode-lz4")(lambda: _encoder("lz4", N.BLOCKS, LZ4))
family("encode-snappy")(lambda: _encoder("snappy", N.BLOCKS, SN))


@family("bgzf-compress")
def _bgzf_compress():
    """members of 65 280 input bytes through the DEFLATE encoder's slots: what gzip reads back, one stream per buffer"""
    import bgzf_model as B
    L = N.lib()
    bufs = [b"", b"a", B._text(3000, 7), B._text(65280, 8), B._text(65281, 9), B._text(140000, 10), bytes(70000), B._text(199999, 11)]

    def run(e, key, cs):
        res, outs = e.batch_host(0, ENC, 0, cs, [L.cj_bgzf_compress_bound(len(b)) for b in cs], N.BGZF)
        for r, o, b in zip(res, outs, cs):
            assert r == len(o) > 0 and gzip.decompress(bytes(o)) == b and B.sizes(bytes(o)) == len(b)
        return [(int(r), zlib.crc32(bytes(o))) for r, o in zip(res, outs)]
    return [("bgzf-enc", bufs, run)]


# d_zstd_slots
@family("zstd-decode")
def _zstd():
    L = N.lib()
    cs = NC.zstd_cases()
    call = lambda e, n: lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, DEC, 0, n, i, o, l, out, oo, oc, r, None))
    return [("zstd", cs, device_run(call)), (("zstd", "host"), NC.shuffled(cs), host_run(lambda e, x: e.batch_host(N.ZSTD_FRAMES, DEC, 0, _raws(x), _caps(x), N.ZSTD)))]


# d_meta, h_meta, h_in, h_out once more: the block decoders' host entry (the engine picks the windows itself)
@family("blocks-host-entry")
def _blocks_host():
    return [(("front", c, "host"), NC.shuffled(NC.front_cases(c)), host_run(lambda e, x, w=w: e.batch_host(w, DEC, 0, _raws(x), _caps(x))))
            for c, w in (("lz4", LZ4), ("snappy", SN))]


# ---- the preparations ------------------------------------------------------------------------------------------------------------------------
def _head(key, cases):
    """the smaller batch of a family: the first 130 cases under a key of its own (the harnesses keep layouts by key)"""
    return ((key, "head", HEAD), cases[:HEAD]) if len(cases) > HEAD else (key, cases)


_cur = {}


def _close():
    if _cur.get("eng") is not None:
        _cur["eng"].close()
    _cur.clear()


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    _close()


def _state(name):
    """the family's engine with its buffers in place — fresh, every batch of the family run once on it — and what those runs computed"""
    if _cur.get("name") != name:
        _close()
        default_engine, make = FAMILIES[name]
        batches = make()
        eng = None if default_engine else N.Engine(0)
        _cur.update(name=name, eng=eng, h=None if default_engine else eng.h, batches=batches)
        _cur["base"] = [run(eng, key, cases) for key, cases, run in batches]
    return _cur


@pytest.mark.parametrize("prep", PREPS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_no_result_depends_on_what_the_scratch_held(name, prep):
    st = _state(name)
    eng = st["eng"]
    if prep != "residue":
        filled = _fill_and_peek(st["h"], PATTERN[prep])
        assert sum(filled.values()) > 0
        for (key, cases, run), base in zip(st["batches"], st["base"]):
            assert run(eng, key, cases) == base, (name, prep, key)
        return
    for (key, cases, run), base in zip(st["batches"], st["base"]):
        if len(cases) > HEAD:                      # the full list, then its first 130 cases
            assert run(eng, key, cases) == base, (name, prep, key)
            assert run(eng, *_head(key, cases)) == base[:HEAD], (name, prep, key, "head")
        else:                                      # a short list: reversed, then in order
            assert run(eng, (key, "reversed"), cases[::-1]) == base[::-1], (name, prep, key, "reversed")
            assert run(eng, key, cases) == base, (name, prep, key)


def test_the_families_reach_every_buffer():
    """the smallest batch of every family on ONE fresh engine, one fill: every listed buffer that is not a state carrier was there to be
    filled — but h_res (this file's head) and, on an engine of its own, d_frame, d_big and d_bigtab, which only the single-buffer API
    reaches: that family runs on the default engine, which is then filled and read back too."""
    _close()
    names, carriers = _names(), _carriers()
    assert carriers == {"h_count"} and NEVER_REACHED <= set(names) and DEFAULT_ENGINE_ONLY <= set(names)
    eng = N.Engine(0)
    try:
        for name, (default_engine, make) in FAMILIES.items():
            for key, cases, run in make():
                run(None if default_engine else eng, *_head(key, cases))
        filled = _fill_and_peek(eng.h, PATTERN["hash"])
    finally:
        eng.close()
    assert set(filled) == set(names)
    missing = [n for n in names if filled[n] == 0 and n not in carriers | NEVER_REACHED | DEFAULT_ENGINE_ONLY]
    assert not missing, missing
    assert all(filled[n] == 0 for n in carriers)
    on_default = _fill_and_peek(None, PATTERN["hash"])
    for n in ("d_frame", "d_big", "d_bigtab", "d_in", "d_out", "d_meta"):
        assert on_default[n] > 0, n
    assert all(on_default[n] == 0 for n in carriers)
