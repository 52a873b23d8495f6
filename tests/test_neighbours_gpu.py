"""The neighbour sweep on the GPU (tests/neighbour_cases.py): every batch decoder, size query and encoder through its
DEVICE entry with its inputs packed under each of the four rings — zeros around every chunk (the older tests' layout, the control),
0xFF, the chunk's own bytes continued (a cut stream's continuation, an encoder input's period), and no gap at all — and, packed by
the library's own staging, once through its HOST entry.  One expected value per case, the reference's on the chunk alone, whatever
the ring: results and bytes (sha256 where the case records one), 64 guard bytes of 0xA5 around every output slot intact, nothing
written behind a result, and the input blob read back unchanged."""
import hashlib

import numpy as np
import pytest

import neighbour_cases as NC
from cramjam_amd import _native as N
from test_capacity_gpu import PATHS

pytestmark = pytest.mark.gpu
G = 64                                             # guard bytes around every output slot
LZ4, SN, DEC, ENC = N.CODEC_LZ4_BLOCK, N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS, N.OP_COMPRESS
WRAP_NAME = ("raw", "zlib", "gzip")
sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd.batch import _engine
    return _engine(0)


_slots = {}


def _out_slots(key, cases):
    """per case list, once: capacities, slot offsets (G bytes of guard around each), the total, and the mask of the output bytes that
    must still be 0xA5 behind the call — all but [0, result) of an accepted chunk and [0, `written` or cap) of a refused one (which
    may have written inside its own slot before it found the stream bad)"""
    if key not in _slots:
        caps = np.array([c["cap"] for c in cases], np.uint64)
        ooff = (G + np.concatenate([[0], np.cumsum(caps + np.uint64(G))[:-1]])).astype(np.uint64)
        total = int(ooff[-1] + caps[-1]) + G + 64
        keep = np.ones(total, bool)
        for lo, c in zip(ooff, cases):
            if not c.get("sized"):                 # (a size query has no output: nothing of the mask is cleared for it)
                keep[int(lo):int(lo) + (c["result"] if c["result"] >= 0 else c.get("written", c["cap"]))] = False
        _slots[key] = caps, ooff, total, keep, np.array([c["result"] for c in cases], np.int64)
    return _slots[key]


def _tag(key, ring, c, got):
    return key, ring, c["base"], "k", c.get("k"), "len", len(c["bytes"]), "cap", c["cap"], "got", int(got), "want", c["result"]


def _device(e, key, cases, ring, call, packed=None, dictionary=None, more=0):
    """one device batch: call(d_in, in_off, in_len, d_out, out_off, out_cap, result[, d_dict]) over the cases packed under `ring`
    (packed: a (blob, offsets) made elsewhere; more: bytes added to every in_len), then every assertion of this file's head"""
    blob, off = packed if packed is not None else NC.case_layout(key, cases, ring)[:2]
    assert not NC.alignment_coverage(cases, off), (key, ring, NC.alignment_coverage(cases, off))
    caps, ooff, total, keep, want = _out_slots(key, cases)
    n = len(cases)
    lens = np.array([len(c["bytes"]) + more for c in cases], np.uint64)
    d_in, d_out, d_meta = e.alloc(blob.nbytes), e.alloc(total), e.alloc(5 * 8 * n)
    d_dict = e.alloc(len(dictionary) + 32) if dictionary is not None else None
    try:
        e.h2d(d_in, blob)
        e.h2d(d_meta, np.concatenate([off, lens, ooff, caps, np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)]))
        N.check(N.lib().cj_memset_dev(e.h, d_out, 0xA5, total))
        m = [d_meta + 8 * n * k for k in range(5)]
        if dictionary is not None:
            e.h2d(d_dict + 3, np.frombuffer(dictionary, np.uint8))                 # (3 bytes off a granule)
            call(d_in, m[0], m[1], d_out, m[2], m[3], m[4], d_dict + 3)
        else:
            call(d_in, m[0], m[1], d_out, m[2], m[3], m[4])
        e.sync()
        res, out, back = e.d2h(m[4], 8 * n, "int64"), e.d2h(d_out, total), e.d2h(d_in, blob.nbytes)
    except N.EngineError as ex:                     # a call or a copy failed on the device: no later test of the session starts another
        pytest.exit("device error in %r under %r: %s" % (key, ring, ex), 1)
    finally:
        for p in (d_in, d_out, d_meta, d_dict):
            if p is not None: e.free(p)
    bad = np.nonzero(res != want)[0]
    assert len(bad) == 0, (len(bad), [_tag(key, ring, cases[i], res[i]) for i in bad[:6]])
    dirty = np.nonzero(out[keep] != 0xA5)[0]
    if len(dirty):                                  # which chunk's neighbourhood: the first byte that changed
        at = int(np.nonzero(keep)[0][dirty[0]])
        i = max(int(np.searchsorted(ooff, at, side="right")) - 1, 0)
        assert False, ("a guard byte or a byte behind the result changed", at - int(ooff[i]), len(dirty), _tag(key, ring, cases[i], res[i]))
    for i in np.nonzero(want > 0)[0]:
        c = cases[i]
        if c.get("sized"):
            continue
        got = out[int(ooff[i]):int(ooff[i]) + int(want[i])]
        assert (got.tobytes() == c["out"]) if c["out"] is not None else (sha(got) == c["sha"]), ("bytes", _tag(key, ring, c, res[i]))
    assert (back == blob).all(), ("the input was written", key, ring)


def _shuffled(cases, seed=20):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


def _host_check(key, cases, res, outs):
    for c, r, o in zip(cases, res, outs):
        assert r == c["result"], _tag(key, "host", c, r)
        assert len(o) == max(r, 0) and (r <= 0 or ((bytes(o) == c["out"]) if c["out"] is not None else (sha(o) == c["sha"]))), ("bytes", _tag(key, "host", c, r))


# ---- decoders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_decode(eng, wrap, ring):
    L = N.lib()
    cs = NC.deflate_cases(wrap)
    assert len(cs) < 40000
    _device(eng, ("deflate", wrap), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(eng.h, wrap, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_size_query(eng, wrap, ring):
    L = N.lib()
    cs = NC.deflate_size_cases(wrap)
    _device(eng, ("deflate-size", wrap), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_sizes_device(eng.h, wrap, 0, len(cs), i, o, l, r, None)))


def test_the_rings_reach_the_device(eng):
    """the control of this file: with every in_len overstated by 3 the ring's first bytes count as stream, and the raw DEFLATE decoder
    then gives what zlib gives on s[:k] + those 3 bytes — under `own`, `ff` and `zero` not the same thing at many cuts.  So the bytes
    the layouts put around a chunk are where the device sees them, and a decoder that used them would be caught above."""
    import deflate_cases as DF
    L = N.lib()
    cuts = NC.at_four_alignments([c for c in NC.deflate_cases(0)[::4] if c["cap"] == 364])      # (one per cut, aligned anew)
    seen = {}
    for ring in ("zero", "ff", "own"):
        _, _, _, behinds = NC.case_layout(("deflate", 0, "+3"), cuts, ring)
        cs = []
        for c, b in zip(cuts, behinds):
            r, o = DF.verdict(0, c["bytes"] + b[:3], c["cap"])
            cs.append(dict(c, result=r, out=o))
            seen.setdefault((c["base"], c["k"], c["mis"]), set()).add((r, o))
        _device(eng, ("deflate", 0, "+3", ring), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(eng.h, 0, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)),
                packed=NC.case_layout(("deflate", 0, "+3"), cuts, ring)[:2], more=3)
    assert 4 * sum(len(v) > 1 for v in seen.values()) >= len(seen)


@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_host_entries(wrap):
    from cramjam_amd import batch
    cs = _shuffled(NC.deflate_cases(wrap)[::4])
    res, outs = batch.deflate_decompress_many([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs], wrapper=WRAP_NAME[wrap])
    _host_check(("deflate", wrap), cs, res, outs)
    cs = _shuffled(NC.deflate_size_cases(wrap)[::4])
    assert batch.deflate_sizes([c["bytes"] for c in cs], wrapper=WRAP_NAME[wrap]) == [c["result"] for c in cs]


@pytest.mark.parametrize("ring", NC.RINGS)
def test_zstd_decode(eng, ring):
    L = N.lib()
    cs = NC.zstd_cases()
    _device(eng, "zstd", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_device(eng.h, N.ZSTD_FRAMES, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


def test_zstd_host_entry():
    from cramjam_amd import batch
    cs = _shuffled(NC.zstd_cases()[::4])
    res, outs = batch._run(N.ZSTD_FRAMES, DEC, 0, [c["bytes"] for c in cs], [c["cap"] for c in cs], None, None, N.ZSTD)
    _host_check("zstd", cs, res, outs)


@pytest.mark.parametrize("ring", NC.RINGS)
def test_lz4_dictionary_decode(eng, ring):
    import lz4_dict_model as D
    L = N.lib()
    cs = NC.lz4_dict_cases()
    call = lambda i, o, l, out, oo, oc, r, d: N.check(L.cj_dict_batch_device(eng.h, LZ4, DEC, 0, len(cs), i, o, l, out, oo, oc, r, d, NC.DICT_LEN, None))
    _device(eng, "lz4-dict", cs, ring, call, dictionary=D.dictionary(NC.DICT_LEN))


def test_lz4_dictionary_host_entry():
    import lz4_dict_model as D
    from cramjam_amd import batch
    cs = _shuffled(NC.lz4_dict_cases())
    res, outs = batch.lz4_decompress_blocks([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs], dictionary=D.dictionary(NC.DICT_LEN))
    _host_check("lz4-dict", cs, res, outs)


def _bgzf_cases():
    """a refused BGZF stream is refused by the walk or for its capacity before a byte is written, or by a member's decoder, which may
    have written inside the slot"""
    return [dict(c, written=0 if c["size"] < 0 or c["size"] > c["cap"] else c["cap"]) for c in NC.bgzf_cases()]


@pytest.mark.parametrize("ring", NC.RINGS)
def test_bgzf_decode(eng, ring):
    L = N.lib()
    cs = _bgzf_cases()
    _device(eng, "bgzf", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(eng.h, 0, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


@pytest.mark.parametrize("ring", NC.RINGS)
def test_bgzf_size_query(eng, ring):
    L = N.lib()
    cs = NC.bgzf_size_cases()
    _device(eng, "bgzf-size", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_sizes_device(eng.h, 0, 0, len(cs), i, o, l, r, None)))


def test_bgzf_host_entries():
    from cramjam_amd import batch
    cs = _shuffled(NC.bgzf_cases())
    res, outs = batch.bgzf_decompress_many([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs])
    _host_check("bgzf", cs, res, outs)
    assert list(batch.bgzf_sizes([c["bytes"] for c in cs])) == [c["size"] for c in cs]


@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("which", ("blosclz", "zcodecs"))
def test_blosc_chunks_decode(eng, which, ring):
    L = N.lib()
    flags, cs = NC.blosc_cases(which)
    _device(eng, ("blosc", which), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_blosc_batch_device(eng.h, 0, i, o, l, out, oo, oc, r, len(cs), None, flags, None)))


@pytest.mark.parametrize("which", ("blosclz", "zcodecs"))
def test_blosc_chunks_host_entry(which):
    """(the host entry takes each chunk's capacity from its own header: the cases whose capacity is that)"""
    from cramjam_amd import batch
    _, cs = NC.blosc_cases(which)
    cs = _shuffled([c for c in cs if len(c["bytes"]) >= 16 and int.from_bytes(c["bytes"][4:8], "little") == c["cap"]])
    assert len(cs) >= 300
    kw = dict(blosclz=True) if which == "blosclz" else dict(blosclz=True, zlib=True, zstd=True)
    res, outs = batch.blosc_decompress_chunks([c["bytes"] for c in cs], **kw)
    _host_check(("blosc", which), cs, res, outs)


@pytest.mark.parametrize("flags,win", PATHS)
@pytest.mark.parametrize("codec", ("lz4", "snappy"))
def test_block_decoders_with_ff_in_front(eng, codec, flags, win):
    """the `own` cuts of the input sweep's family A, body a — the stream's continuation behind every cut, as there — with 48 bytes of
    0xFF in front of every chunk, through every decoder path"""
    cs = NC.front_cases(codec)
    _device(eng, ("front", codec), cs, "own", lambda i, o, l, out, oo, oc, r: eng.batch_device(LZ4 if codec == "lz4" else SN, DEC, flags, len(cs), i, o, l, out, oo, oc, r))


# ---- encoders ------------------------------------------------------------------------------------------------------------------------------
def _encode_call(eng, codec, n):
    L = N.lib()
    if codec in ("lz4", "snappy"):
        return lambda i, o, l, out, oo, oc, r: eng.batch_device(LZ4 if codec == "lz4" else SN, ENC, 0, n, i, o, l, out, oo, oc, r)
    if codec == "lz4_dict":
        return lambda i, o, l, out, oo, oc, r, d: N.check(L.cj_dict_batch_device(eng.h, LZ4, ENC, 0, n, i, o, l, out, oo, oc, r, d, NC.DICT_LEN, None))
    if codec.startswith("deflate"):
        wrap = NC.ENCODERS.index(codec) - 3
        return lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_compress_batch_device(eng.h, wrap, 0, n, i, o, l, out, oo, oc, r, None))
    return lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_compress_batch_device(eng.h, N.ZSTD_FRAMES, 0, n, i, o, l, out, oo, oc, r, None))


@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("codec", NC.ENCODERS)
def test_encoders_emit_the_models_bytes(eng, codec, ring):
    """periodic inputs of every period and length flanked by their own period, and text followed by its own last bytes: a match
    measured past n, or backward below position 0, finds bytes that match — and must not use them"""
    import lz4_dict_model as D
    cs = NC.encoder_cases(codec)
    _device(eng, ("enc", codec), cs, ring, _encode_call(eng, codec, len(cs)), dictionary=D.dictionary(NC.DICT_LEN) if codec == "lz4_dict" else None)


@pytest.mark.parametrize("codec", NC.ENCODERS)
def test_encoders_host_entries(eng, codec):
    import lz4_dict_model as D
    from cramjam_amd import batch
    cs = _shuffled(NC.encoder_cases(codec))
    raws = [c["bytes"] for c in cs]
    if codec in ("lz4", "snappy"):
        res, outs = eng.batch_host(LZ4 if codec == "lz4" else SN, ENC, 0, raws, [c["cap"] for c in cs])
    elif codec == "lz4_dict":
        res, outs = batch.lz4_compress_blocks(raws, store_size=False, dictionary=D.dictionary(NC.DICT_LEN))
    elif codec.startswith("deflate"):
        res, outs = batch.deflate_compress_many(raws, wrapper=WRAP_NAME[NC.ENCODERS.index(codec) - 3])
    else:
        res, outs = batch.zstd_compress_many(raws)
    _host_check(("enc", codec), cs, res, outs)
