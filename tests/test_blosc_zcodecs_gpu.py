"""Zlib and Zstd streams in Blosc chunks on the GPU (CJ_BLOSC_FLAG_READ_ZLIB / _ZSTD; zlib=True, zstd=True): the fixtures c-blosc
minted through every decode entry, one batch that interleaves LZ4, BloscLZ, Zlib and Zstd chunks into slots packed without a gap,
malformed and hand-made chunks between intact neighbours of another format, the Zstandard launcher's slot slices inside a chunk's
streams, and the default reading, which still refuses both formats.  Fixtures only: the verdict classes and sha256 recorded in
tests/golden/golden_blosc_zcodecs.json, neither the model nor libzstd nor libblosc."""
import os

import numpy as np
import pytest

import blosc_cases as K
import blosc_model as M
import blosc_zcodec_model as Z
import device_batch as DB

pytestmark = pytest.mark.gpu

ALL = 2 | Z.FLAGS                       # CJ_BLOSC_FLAG_READ_BLOSCLZ | _ZLIB | _ZSTD
KW = dict(zlib=True, zstd=True)


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def test_fixtures_single_chunk_with_the_flags():
    from cramjam_amd import blosc2
    for v in Z.valid():
        out = blosc2.decompress_chunk(v["bytes"], **KW)
        assert len(out) == v["nbytes"] and Z.sha(out) == v["sha256"], v["name"]
        buf = bytearray(v["nbytes"] + 5)
        assert blosc2.decompress_chunk_into(v["bytes"], buf, **KW) == v["nbytes"] and Z.sha(buf[:v["nbytes"]]) == v["sha256"], v["name"]
        assert bytes(buf[v["nbytes"]:]) == bytes(5), v["name"]


def test_fixtures_host_batch_with_the_flags():
    from cramjam_amd import batch
    vs = Z.valid()
    order = np.random.default_rng(5).permutation(len(vs))
    chunks = [vs[i]["bytes"] for i in order]
    sizes = batch.blosc_chunk_sizes(chunks, **KW)
    assert sizes == [vs[i]["nbytes"] for i in order]
    res, outs = batch.blosc_decompress_chunks(chunks, **KW)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] == len(outs[k]) and Z.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]
    buf = bytearray(sum(sizes))
    res, outs = batch.blosc_decompress_chunks(chunks, out=buf, **KW)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] == len(outs[k]) and Z.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]


def test_fixtures_device_batch_on_a_side_stream():
    """the device-resident entries on torch tensors, in a child that imports torch BEFORE cramjam_amd (tests/device_api_child.py says why)"""
    DB.run_child(os.path.join(K.ROOT, "tests", "blosc_zcodecs_torch_child.py"), "fixtures: ok", 600)


def _four_formats():
    """LZ4, BloscLZ, Zlib and Zstd fixtures interleaved: [(fixture, compressor format of its streams or None)]"""
    import blosclz_model as B
    zs = Z.valid()
    lists = [K.valid(), B.valid(), [v for v in zs if v["recipe"]["cname"] == "zlib"], [v for v in zs if v["recipe"]["cname"] == "zstd"]]
    vs = []
    for k in range(max(len(x) for x in lists)):
        for x in lists:
            vs += x[k:k + 1]
    assert len(vs) == sum(len(x) for x in lists)

    def fmt(v):
        b = v["bytes"]
        return None if len(b) < 16 or b[2] & 2 or v["nbytes"] == 0 else b[2] >> 5
    return [(v, fmt(v)) for v in vs]


def test_one_batch_interleaves_the_four_formats_into_packed_slots(eng):
    e, N = eng
    vf = _four_formats()
    assert {f for _v, f in vf} == {None, 0, 1, 3, 4}
    vs = [v for v, _f in vf]
    sizes = [v["nbytes"] for v in vs]
    res, out, ooff = K.device_batch(e, N, [v["bytes"] for v in vs], sizes, sizes, ALL)       # slot = nbytes: no gap, whatever the alignment
    assert [int(o) for o in ooff] == [sum(sizes[:i]) for i in range(len(vs))]
    for i, v in enumerate(vs):
        lo = int(ooff[i])
        assert res[i] == v["nbytes"] and Z.sha(out[lo:lo + v["nbytes"]]) == v["sha256"], (i, v["name"], res[i])
    end = sum(sizes)
    assert len(out) >= end + 64 and (out[end:end + 64] == 0xA5).all()


def test_the_same_batch_with_the_zlib_flag_alone(eng):
    """the Zstd and BloscLZ chunks are refused (-31) and write nothing, the LZ4 and Zlib chunks decode"""
    e, N = eng
    vf = _four_formats()
    vs = [v for v, _f in vf]
    sizes = [v["nbytes"] for v in vs]
    res, out, ooff = K.device_batch(e, N, [v["bytes"] for v in vs], sizes, sizes, Z.FLAG_ZLIB)
    refused = 0
    for i, (v, f) in enumerate(vf):
        lo = int(ooff[i])
        if f in (0, 4):
            assert res[i] == -31 and (out[lo:lo + v["nbytes"]] == 0xA5).all(), (i, v["name"], res[i])
            refused += 1
        else:
            assert res[i] == v["nbytes"] and Z.sha(out[lo:lo + v["nbytes"]]) == v["sha256"], (i, v["name"], res[i])
    assert refused >= 100
    end = sum(sizes)
    assert (out[end:end + 64] == 0xA5).all()


def test_malformed_and_hand_made_chunks_between_intact_neighbours_of_another_format(eng):
    e, N = eng
    zs = Z.valid()
    pick = lambda cname: next(v for v in zs if v["recipe"]["cname"] == cname and v["nbytes"] == 4096 and Z.fmt_of(v["bytes"]) and v["bytes"][3] == 8)
    lz4 = next(x for x in K.valid() if 4000 <= x["nbytes"] <= 70000)
    neighbours = {Z.FORMAT_ZLIB: [pick("zstd"), lz4], Z.FORMAT_ZSTD: [pick("zlib"), lz4]}      # of another format than the case between them
    cases = Z.malformed() + Z.hand()
    assert {c["verdict"] for c in cases} == {"ok", M.CORRUPT, M.HEADER, M.UNSUPPORTED, M.TOO_SMALL}
    chunks, expect = [], []
    for k, c in enumerate(cases):
        fmt = Z.FORMAT_ZLIB if c["name"].startswith("zlib") else Z.FORMAT_ZSTD
        g = neighbours[fmt][k % 2]
        chunks += [g["bytes"], c["bytes"]]
        expect += [(g, g["nbytes"]), (c, c["cap"])]
    g = neighbours[Z.FORMAT_ZLIB][0]
    chunks.append(g["bytes"]); expect.append((g, g["nbytes"]))
    G = 64
    caps = [cap for _x, cap in expect]
    slots = [(c + 15) // 16 * 16 for c in caps]
    res, out, ooff = K.device_batch(e, N, chunks, caps, slots, ALL, guard=G)
    for i, (x, cap) in enumerate(expect):
        lo = int(ooff[i])
        cls = x.get("verdict", "ok")
        if cls == "ok":
            assert res[i] == x["nbytes"] and Z.sha(out[lo:lo + x["nbytes"]]) == x["sha256"], (i, x["name"], res[i])
            used = x["nbytes"]
        else:
            assert res[i] == M.CODE[cls], (x["name"], res[i], cls)
            # refused from its header or for its size: nothing written; a bad stream shows only after other bytes of the chunk were
            # written: nothing outside the slot
            used = cap if cls == M.CORRUPT else 0
        assert (out[lo + used:lo + slots[i] + G] == 0xA5).all() and (out[lo - G:lo] == 0xA5).all(), (i, x["name"])


def test_zstd_slot_slices_fall_inside_a_chunks_streams(eng):
    """cj_debug_zstd_slot_budget lowered to three literal slots: a batch of split Zstd chunks (four streams each) goes through the
    Zstandard launcher in slices of three rows, whose borders fall inside the chunks; the results equal the unsliced run's"""
    e, N = eng
    vs = [v for v in Z.valid() if Z.fmt_of(v["bytes"]) == Z.FORMAT_ZSTD and not v["bytes"][2] & 16 and v["bytes"][3] == 4 and v["nbytes"] >= 20000]
    vs = (vs * 2)[:8]
    assert len(vs) >= 4 and sum(len(Z.parse(v["bytes"])[1]) for v in vs) >= 16
    sizes = [v["nbytes"] for v in vs]
    chunks = [v["bytes"] for v in vs]
    whole = K.device_batch(e, N, chunks, sizes, sizes, Z.FLAG_ZSTD)
    L = N.lib()
    slot = 131072 + 32                                                 # kZsSlotBytes
    prev = L.cj_debug_zstd_slot_budget(3 * slot)
    try:
        sliced = K.device_batch(e, N, chunks, sizes, sizes, Z.FLAG_ZSTD)
    finally:
        assert L.cj_debug_zstd_slot_budget(prev) == 3 * slot
    assert list(whole[0]) == list(sliced[0]) == sizes and (whole[1] == sliced[1]).all()
    for i, v in enumerate(vs):
        lo = int(sliced[2][i])
        assert Z.sha(sliced[1][lo:lo + v["nbytes"]]) == v["sha256"], v["name"]


def test_default_reading_still_refuses_both_formats():
    from cramjam_amd import batch, blosc2
    vs = Z.valid()
    refused = [Z.fmt_of(v["bytes"]) is not None for v in vs]        # (memcpyed and empty chunks carry no stream: they are read whatever their format)
    assert sum(refused) >= 70 and not all(refused)
    for v, r in zip(vs[::7], refused[::7]):
        if r:
            with pytest.raises(Exception) as ex:
                blosc2.decompress_chunk(v["bytes"])
            assert "unsupported" in str(ex.value), v["name"]
            with pytest.raises(Exception) as ex:
                blosc2.decompress_chunk_into(v["bytes"], bytearray(v["nbytes"]), blosclz=True)
            assert "unsupported" in str(ex.value), v["name"]
        else:
            assert Z.sha(blosc2.decompress_chunk(v["bytes"])) == v["sha256"], v["name"]
    chunks = [v["bytes"] for v in vs]
    for kw in ({}, dict(blosclz=True)):
        assert batch.blosc_chunk_sizes(chunks, **kw) == [-31 if r else v["nbytes"] for v, r in zip(vs, refused)]
        res, outs = batch.blosc_decompress_chunks(chunks, **kw)
        for v, r, got, o in zip(vs, refused, res, outs):
            assert got == (-31 if r else v["nbytes"]) and len(o) == (0 if r else v["nbytes"]), v["name"]
