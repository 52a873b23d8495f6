"""The engine's size classes as the containers pick them (cramjam_amd/csrc/cj_codecs.hpp: size_class_flags): LZ4 and
Snappy entries of ORC streams, Parquet chunks and Blosc chunks whose largest entry is exactly L bytes, for L on both sides of the three
class edges — 16 KiB, 32 KiB and 64 KiB.  Every batch has three streams: one whose largest entry is L bytes of text, one whose largest
entry is L incompressible bytes — its compressed form is LONGER than L, which is what routes a row out of its class's decoder — and one
of entries of 1 and 4096 bytes.  The compressed entries are the oracle's, framed by the models' writers; before anything runs on the
device the models must accept every case with the decoded length as their verdict.

Blosc: typesize 1 runs without a filter and with shuffle, but shuffle never transposes a block of typesize 1 (c-blosc shuffles only for
typesize > 1: blosc_block_mode), so both give DIRECT streams.  Typesize 2 with shuffle, unsplit, runs next to them: those blocks are
transposed, their streams of L bytes decode into the scratch."""
import struct

import numpy as np
import pytest

import blosc_model as BM
import deflate_cases as D
import device_batch as DB
import orc_model as OM
import parquet_model as PM

EDGES = (16384, 16385, 32768, 32769, 65536, 65537)
CODECS = ("lz4", "snappy")
BLOSC = {"nofilter-t1": (1, 0), "shuffle-t1": (1, 1), "shuffle-t2": (2, 1)}      # (typesize, filter flag)
gpu = pytest.mark.gpu

_text, _small = D.words(65537, 97), D.words(4097, 98)
_rnd = np.random.default_rng(30).integers(0, 256, 65537, dtype=np.uint8).tobytes()
_comp = {}


def entries(L):
    """the decoded entries of the three streams"""
    return [_text[:L]], [_rnd[:L]], [_small[:1], _small[1:]]


def comp(codec, raw):
    """the oracle's LZ4 block / Snappy raw stream of `raw`, decoded back once"""
    import oracle
    key = (codec, raw)
    if key not in _comp:
        r, c = (oracle.lz4_compress_raw if codec == "lz4" else oracle.snappy_compress)(raw)
        assert r == len(c) > 0
        assert (oracle.lz4_decompress_raw(c, len(raw)) if codec == "lz4" else oracle.snappy_decompress(c)) == (len(raw), raw)
        _comp[key] = c
    return _comp[key]


def check_shapes(codec, L):
    t, r, s = entries(L)
    assert len(t[0]) == len(r[0]) == L and [len(x) for x in s] == [1, 4096]
    assert len(comp(codec, t[0])) < L < len(comp(codec, r[0]))


# ---- the cases: (inputs, decoded bytes) per container, the model's verdict asserted ------------------------------------------------------------
def orc_cases(codec, L):
    check_shapes(codec, L)
    ins = []
    for es in entries(L):
        s = OM.frame([(0, comp(codec, x)) for x in es])
        sizes = [len(x) for x in es]
        assert OM.verdict(OM.walk(s)[0], sizes, L, sum(sizes)) == OM.verdict(OM.walk(s)[0], sizes, L) == sum(sizes)
        ins.append(s)
    return ins, [b"".join(es) for es in entries(L)]


def parquet_cases(codec, L):
    check_shapes(codec, L)
    name = "lz4_raw" if codec == "lz4" else codec
    ins = []
    for es in entries(L):
        chunk = b"".join(PM.page(comp(codec, x), len(x)) for x in es)
        total = sum(len(x) for x in es)
        assert PM.verdict(chunk, name, total, verify_crc=True) == PM.verdict(chunk, name) == total
        ins.append(chunk)
    return ins, [b"".join(es) for es in entries(L)]


def blosc_chunk(raw, blocksize, typesize, filt):
    """a Blosc1 chunk of LZ4 streams, one stream per block (flag 0x10: unsplit)"""
    flags = filt | 0x10 | 1 << 5
    nblocks = -(-len(raw) // blocksize)
    body, bstarts = b"", []
    for at in range(0, len(raw), blocksize):
        blk = raw[at:at + blocksize]
        c = comp("lz4", BM.apply_filter(blk, typesize, BM.block_mode(flags, typesize, len(blk)), True))
        assert len(c) != len(blk)                                     # (that would read as a stored stream)
        bstarts.append(16 + 4 * nblocks + len(body))
        body += struct.pack("<i", len(c)) + c
    return struct.pack("<BBBBIII", 2, 1, flags, typesize, len(raw), blocksize, 16 + 4 * nblocks + len(body)) + struct.pack("<%dI" % nblocks, *bstarts) + body


def blosc_cases(how, L):
    check_shapes("lz4", L)
    typesize, filt = BLOSC[how]
    raws = [b"".join(es) for es in entries(L)]
    ins = [blosc_chunk(raw, bs, typesize, filt) for raw, bs in zip(raws, (L, L, 4096))]
    for chunk, raw, longest in zip(ins, raws, (L, L, 4096)):
        h, streams = BM.parse(chunk)
        assert BM.decode(chunk, len(raw)) == raw and max(s[3] for s in streams) == longest
        assert all(BM.block_mode(h["flags"], typesize, s[3]) == (1 if how == "shuffle-t2" else 0) for s in streams)
    assert len(ins[1]) > L + 16
    return ins, raws


def test_the_models_accept_every_case():
    for L in EDGES:
        for codec in CODECS:
            orc_cases(codec, L)
            parquet_cases(codec, L)
        for how in BLOSC:
            blosc_cases(how, L)


# ---- the device ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def run(e, tag, ins, raws, decode, sizes, mis=DB.in_mis, out_mis=DB.out_mis):
    """one guarded decode batch and one size query over the same inputs: the decoded lengths, the bytes, nothing outside them"""
    blob, off, lens = DB.pack(ins, mis=mis)
    want = np.array([len(r) for r in raws], np.int64)
    caps = want.astype(np.uint64)
    ooff, total = DB.out_slots(caps, mis=out_mis)
    res, out, blob_after = DB.run(e, decode, blob, off, lens, ooff, caps, total, with_input=True, what=tag)
    DB.check_results(res, want, lambda i: tag + (i, int(res[i])))
    DB.check_mask(out, DB.untouched(ooff, want, total), ooff, lambda i: tag + (i,))
    assert DB.guards_intact(out, ooff, caps) is None and (blob_after == blob).all()
    for i, r in enumerate(raws):
        assert out[int(ooff[i]):int(ooff[i]) + len(r)].tobytes() == r, ("bytes",) + tag + (i,)
    res, out = DB.run(e, sizes, blob, off, lens, ooff, caps, total, what=tag + ("sizes",))
    DB.check_results(res, want, lambda i: tag + ("sizes", i, int(res[i])))
    assert (out == DB.FILL).all()


@gpu
@pytest.mark.parametrize("L", EDGES)
@pytest.mark.parametrize("codec", CODECS)
def test_orc_block_size_at_the_class_edges(eng, codec, L):
    e, N = eng
    lib, kind = N.lib(), OM.KINDS[codec]
    ins, raws = orc_cases(codec, L)
    n = len(ins)
    run(e, ("orc", codec, L), ins, raws,
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_orc_batch_device(e.h, kind, N.OP_DECOMPRESS, 0, L, n, i, o, l, out, oo, oc, r, None)),
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_orc_sizes_device(e.h, kind, 0, L, n, i, o, l, r, None)))


@gpu
@pytest.mark.parametrize("L", EDGES)
@pytest.mark.parametrize("codec", CODECS)
def test_parquet_largest_page_at_the_class_edges(eng, codec, L):
    e, N = eng
    lib, what = N.lib(), PM.CODECS["lz4_raw" if codec == "lz4" else codec]
    ins, raws = parquet_cases(codec, L)
    n = len(ins)
    run(e, ("parquet", codec, L), ins, raws,
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_parquet_batch_device(e.h, what, N.OP_DECOMPRESS, N.PARQUET_FLAG_VERIFY_CRC, n, i, o, l, out, oo, oc, r, None)),
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_parquet_sizes_device(e.h, what, 0, n, i, o, l, r, None)))


@gpu
@pytest.mark.parametrize("L", EDGES)
@pytest.mark.parametrize("how", tuple(BLOSC))
def test_blosc_longest_stream_at_the_class_edges(eng, how, L):
    e, N = eng
    lib = N.lib()
    ins, raws = blosc_cases(how, L)
    n = len(ins)
    run(e, ("blosc", how, L), ins, raws,
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_blosc_batch_device(e.h, N.OP_DECOMPRESS, i, o, l, out, oo, oc, r, n, None, 0, None)),
        lambda i, o, l, out, oo, oc, r: N.check(lib.cj_blosc_chunk_sizes_device(e.h, 0, n, i, o, l, r, None)),
        mis=0, out_mis=None)            # (chunks and slots laid out as tests/blosc_cases.py lays them out)
