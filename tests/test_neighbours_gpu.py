"""The neighbour sweep on the GPU (tests/neighbour_cases.py): every batch decoder, size query and encoder through its
DEVICE entry with its inputs packed under each of the four rings — zeros around every chunk (the older tests' layout, the control),
0xFF, the chunk's own bytes continued (a cut stream's continuation, an encoder input's period), and no gap at all — and, packed by
the library's own staging, once through its HOST entry.  One expected value per case, the reference's on the chunk alone, whatever
the ring: results and bytes (sha256 where the case records one), 64 guard bytes of 0xA5 around every output slot intact, nothing
written behind a result, and the input blob read back unchanged."""
import pytest

import neighbour_cases as NC
from capacity_cases import PATHS
from cramjam_amd import _native as N

pytestmark = pytest.mark.gpu
LZ4, SN, DEC, ENC = N.CODEC_LZ4_BLOCK, N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS, N.OP_COMPRESS
WRAP_NAME = ("raw", "zlib", "gzip")


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd.batch import _engine
    return _engine(0)


# ---- decoders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_decode(eng, wrap, ring):
    L = N.lib()
    cs = NC.deflate_cases(wrap)
    assert len(cs) < 40000
    NC.device(eng, ("deflate", wrap), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(eng.h, wrap, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_size_query(eng, wrap, ring):
    L = N.lib()
    cs = NC.deflate_size_cases(wrap)
    NC.device(eng, ("deflate-size", wrap), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_sizes_device(eng.h, wrap, 0, len(cs), i, o, l, r, None)))


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
        NC.device(eng, ("deflate", 0, "+3", ring), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_deflate_batch_device(eng.h, 0, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)),
                packed=NC.case_layout(("deflate", 0, "+3"), cuts, ring)[:2], more=3)
    assert 4 * sum(len(v) > 1 for v in seen.values()) >= len(seen)


@pytest.mark.parametrize("wrap", (0, 1, 2))
def test_deflate_host_entries(wrap):
    from cramjam_amd import batch
    cs = NC.shuffled(NC.deflate_cases(wrap)[::4])
    res, outs = batch.deflate_decompress_many([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs], wrapper=WRAP_NAME[wrap])
    NC.host_check(("deflate", wrap), cs, res, outs)
    cs = NC.shuffled(NC.deflate_size_cases(wrap)[::4])
    assert batch.deflate_sizes([c["bytes"] for c in cs], wrapper=WRAP_NAME[wrap]) == [c["result"] for c in cs]


@pytest.mark.parametrize("ring", NC.RINGS)
def test_zstd_decode(eng, ring):
    L = N.lib()
    cs = NC.zstd_cases()
    NC.device(eng, "zstd", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_zstd_batch_device(eng.h, N.ZSTD_FRAMES, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


def test_zstd_host_entry():
    from cramjam_amd import batch
    cs = NC.shuffled(NC.zstd_cases()[::4])
    res, outs = batch._run(N.ZSTD_FRAMES, DEC, 0, [c["bytes"] for c in cs], [c["cap"] for c in cs], None, None, N.ZSTD)
    NC.host_check("zstd", cs, res, outs)


@pytest.mark.parametrize("ring", NC.RINGS)
def test_lz4_dictionary_decode(eng, ring):
    import lz4_dict_model as D
    L = N.lib()
    cs = NC.lz4_dict_cases()
    call = lambda i, o, l, out, oo, oc, r, d: N.check(L.cj_dict_batch_device(eng.h, LZ4, DEC, 0, len(cs), i, o, l, out, oo, oc, r, d, NC.DICT_LEN, None))
    NC.device(eng, "lz4-dict", cs, ring, call, dictionary=D.dictionary(NC.DICT_LEN))


def test_lz4_dictionary_host_entry():
    import lz4_dict_model as D
    from cramjam_amd import batch
    cs = NC.shuffled(NC.lz4_dict_cases())
    res, outs = batch.lz4_decompress_blocks([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs], dictionary=D.dictionary(NC.DICT_LEN))
    NC.host_check("lz4-dict", cs, res, outs)


@pytest.mark.parametrize("ring", NC.RINGS)
def test_bgzf_decode(eng, ring):
    L = N.lib()
    cs = NC.bgzf_decode_cases()
    NC.device(eng, "bgzf", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(eng.h, 0, DEC, 0, len(cs), i, o, l, out, oo, oc, r, None)))


@pytest.mark.parametrize("ring", NC.RINGS)
def test_bgzf_size_query(eng, ring):
    L = N.lib()
    cs = NC.bgzf_size_cases()
    NC.device(eng, "bgzf-size", cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_sizes_device(eng.h, 0, 0, len(cs), i, o, l, r, None)))


def test_bgzf_host_entries():
    from cramjam_amd import batch
    cs = NC.shuffled(NC.bgzf_cases())
    res, outs = batch.bgzf_decompress_many([c["bytes"] for c in cs], output_lens=[c["cap"] for c in cs])
    NC.host_check("bgzf", cs, res, outs)
    assert list(batch.bgzf_sizes([c["bytes"] for c in cs])) == [c["size"] for c in cs]


@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("which", ("blosclz", "zcodecs"))
def test_blosc_chunks_decode(eng, which, ring):
    L = N.lib()
    flags, cs = NC.blosc_cases(which)
    NC.device(eng, ("blosc", which), cs, ring, lambda i, o, l, out, oo, oc, r: N.check(L.cj_blosc_batch_device(eng.h, 0, i, o, l, out, oo, oc, r, len(cs), None, flags, None)))


@pytest.mark.parametrize("which", ("blosclz", "zcodecs"))
def test_blosc_chunks_host_entry(which):
    """(the host entry takes each chunk's capacity from its own header: the cases whose capacity is that)"""
    from cramjam_amd import batch
    _, cs = NC.blosc_cases(which)
    cs = NC.shuffled([c for c in cs if len(c["bytes"]) >= 16 and int.from_bytes(c["bytes"][4:8], "little") == c["cap"]])
    assert len(cs) >= 300
    kw = dict(blosclz=True) if which == "blosclz" else dict(blosclz=True, zlib=True, zstd=True)
    res, outs = batch.blosc_decompress_chunks([c["bytes"] for c in cs], **kw)
    NC.host_check(("blosc", which), cs, res, outs)


@pytest.mark.parametrize("flags,win", PATHS)
@pytest.mark.parametrize("codec", ("lz4", "snappy"))
def test_block_decoders_with_ff_in_front(eng, codec, flags, win):
    """the `own` cuts of the input sweep's family A, body a — the stream's continuation behind every cut, as there — with 48 bytes of
    0xFF in front of every chunk, through every decoder path"""
    cs = NC.front_cases(codec)
    NC.device(eng, ("front", codec), cs, "own", lambda i, o, l, out, oo, oc, r: eng.batch_device(LZ4 if codec == "lz4" else SN, DEC, flags, len(cs), i, o, l, out, oo, oc, r))


# ---- encoders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", NC.RINGS)
@pytest.mark.parametrize("codec", NC.ENCODERS)
def test_encoders_emit_the_models_bytes(eng, codec, ring):
    """periodic inputs of every period and length flanked by their own period, and text followed by its own last bytes: a match
    measured past n, or backward below position 0, finds bytes that match — and must not use them"""
    import lz4_dict_model as D
    cs = NC.encoder_cases(codec)
    NC.device(eng, ("enc", codec), cs, ring, NC.encode_call(eng, codec, len(cs)), dictionary=D.dictionary(NC.DICT_LEN) if codec == "lz4_dict" else None)


@pytest.mark.parametrize("codec", NC.ENCODERS)
def test_encoders_host_entries(eng, codec):
    import lz4_dict_model as D
    from cramjam_amd import batch
    cs = NC.shuffled(NC.encoder_cases(codec))
    raws = [c["bytes"] for c in cs]
    if codec in ("lz4", "snappy"):
        res, outs = eng.batch_host(LZ4 if codec == "lz4" else SN, ENC, 0, raws, [c["cap"] for c in cs])
    elif codec == "lz4_dict":
        res, outs = batch.lz4_compress_blocks(raws, store_size=False, dictionary=D.dictionary(NC.DICT_LEN))
    elif codec.startswith("deflate"):
        res, outs = batch.deflate_compress_many(raws, wrapper=WRAP_NAME[NC.ENCODERS.index(codec) - 3])
    else:
        res, outs = batch.zstd_compress_many(raws)
    NC.host_check(("enc", codec), cs, res, outs)
