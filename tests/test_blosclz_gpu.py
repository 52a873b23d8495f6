"""BloscLZ streams in Blosc chunks on the GPU (CJ_BLOSC_FLAG_READ_BLOSCLZ / blosclz=True): the fixtures c-blosc minted through every
decode entry, one batch that mixes them with the LZ4 fixtures into slots packed without a gap, malformed and hand-written streams
between intact neighbours, and the default reading, which still refuses them."""
import os

import numpy as np
import pytest

import blosc_cases as K
import blosc_model as M
import blosclz_model as Z
import device_batch as DB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def test_fixtures_single_chunk_with_the_flag():
    from cramjam_amd import blosc2
    for v in Z.valid():
        out = blosc2.decompress_chunk(v["bytes"], blosclz=True)
        assert len(out) == v["nbytes"] and Z.sha(out) == v["sha256"], v["name"]
        buf = bytearray(v["nbytes"] + 5)
        assert blosc2.decompress_chunk_into(v["bytes"], buf, blosclz=True) == v["nbytes"] and Z.sha(buf[:v["nbytes"]]) == v["sha256"], v["name"]
        assert bytes(buf[v["nbytes"]:]) == bytes(5), v["name"]


def test_fixtures_host_batch_with_the_flag():
    from cramjam_amd import batch
    vs = Z.valid()
    order = np.random.default_rng(4).permutation(len(vs))
    chunks = [vs[i]["bytes"] for i in order]
    sizes = batch.blosc_chunk_sizes(chunks, blosclz=True)
    assert sizes == [vs[i]["nbytes"] for i in order]
    res, outs = batch.blosc_decompress_chunks(chunks, blosclz=True)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] == len(outs[k]) and Z.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]
    buf = bytearray(sum(sizes))
    res, outs = batch.blosc_decompress_chunks(chunks, out=buf, blosclz=True)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] == len(outs[k]) and Z.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]


def test_fixtures_device_batch_on_a_side_stream():
    """the device-resident entries on torch tensors, in a child that imports torch BEFORE cramjam_amd (tests/device_api_child.py says why)"""
    DB.run_child(os.path.join(K.ROOT, "tests", "blosclz_torch_child.py"), "fixtures: ok", 600)


def test_one_batch_mixes_lz4_and_blosclz_chunks_into_packed_slots(eng):
    e, N = eng
    lz4, blz = K.valid(), Z.valid()
    vs = []
    for k in range(max(len(lz4), len(blz))):                         # interleaved
        vs += lz4[k:k + 1] + blz[k:k + 1]
    assert len(vs) == len(lz4) + len(blz)
    sizes = [v["nbytes"] for v in vs]
    res, out, ooff = K.device_batch(e, N, [v["bytes"] for v in vs], sizes, sizes, Z.FLAG)       # slot = nbytes: no gap, whatever the alignment
    assert [int(o) for o in ooff] == [sum(sizes[:i]) for i in range(len(vs))]
    for i, v in enumerate(vs):
        lo = int(ooff[i])
        assert res[i] == v["nbytes"] and Z.sha(out[lo:lo + v["nbytes"]]) == v["sha256"], (i, v["name"], res[i])
    end = sum(sizes)
    assert len(out) >= end + 64 and (out[end:end + 64] == 0xA5).all()


def _header_cases():
    """chunks refused from their header or for their size with the flag on: (name, bytes, capacity, class)"""
    v = next(x for x in Z.valid() if x["nbytes"] == 70000 and Z.is_blosclz(x["bytes"]))
    c = v["bytes"]
    return [("versionlz2", M.mutate(c, ["put", 1, "<B", 2]), 70000, M.UNSUPPORTED),
            ("format-zstd", M.mutate(c, ["put", 2, "<B", (c[2] & 31) | (4 << 5)]), 70000, M.UNSUPPORTED),
            ("cut", c[:len(c) // 2], 70000, M.HEADER),
            ("reserved-bit", M.mutate(c, ["put", 2, "<B", c[2] | 8]), 70000, M.HEADER),
            ("capacity-1", c, 69999, M.TOO_SMALL)]


def test_malformed_and_hand_written_streams_between_intact_neighbours(eng):
    e, N = eng
    good = [next(x for x in Z.valid() if x["nbytes"] == 4096 and Z.is_blosclz(x["bytes"])), next(x for x in K.valid() if 4000 <= x["nbytes"] <= 70000)]
    cases = []                                                      # (name, bytes, capacity, class, expected bytes)
    for m in Z.malformed():
        cases.append((m["name"], m["bytes"], 70000, m["verdict"], None))
    for h in Z.hand_chunks():
        cases.append((h["name"], h["bytes"], int.from_bytes(h["bytes"][4:8], "little"), h["verdict"], h["out"]))
    for name, b, cap, cls in _header_cases():
        cases.append((name, b, cap, cls, None))
    assert {c[3] for c in cases} == {"ok", M.CORRUPT, M.HEADER, M.UNSUPPORTED, M.TOO_SMALL}
    chunks, expect = [], []
    for k, c in enumerate(cases):
        g = good[k % 2]
        chunks += [g["bytes"], c[1]]
        expect += [("ok", g, g["nbytes"]), (c[3], c, c[2])]
    G = 64
    caps = [x[2] for x in expect]
    slots = [(c + 15) // 16 * 16 for c in caps]
    res, out, ooff = K.device_batch(e, N, chunks, caps, slots, Z.FLAG, guard=G)
    for i, (cls, x, cap) in enumerate(expect):
        lo = int(ooff[i])
        if isinstance(x, dict):                                      # an intact neighbour
            assert res[i] == x["nbytes"] and Z.sha(out[lo:lo + cap]) == x["sha256"], (i, x["name"], res[i])
            used = cap
        elif cls == "ok":
            want = x[4] if x[4] is not None else Z.decode(x[1])
            assert res[i] == len(want) and out[lo:lo + len(want)].tobytes() == want, (x[0], res[i])
            used = len(want)
        else:
            assert res[i] == M.CODE[cls], (x[0], res[i], cls)
            # refused from its header or for its size: nothing written; a bad stream shows only after other bytes of the chunk were
            # written: nothing outside the slot
            used = cap if cls == M.CORRUPT else 0
        name = x["name"] if isinstance(x, dict) else x[0]
        assert (out[lo + used:lo + slots[i] + G] == 0xA5).all() and (out[lo - G:lo] == 0xA5).all(), (i, name)


def test_default_reading_still_refuses_blosclz_chunks():
    from cramjam_amd import batch, blosc2
    vs = Z.valid()
    refused = [Z.is_blosclz(v["bytes"]) for v in vs]                # (memcpyed chunks carry no stream: they are read whatever their format)
    assert sum(refused) >= 60 and not all(refused)
    for v, r in zip(vs[::5], refused[::5]):
        if r:
            with pytest.raises(Exception) as ex:
                blosc2.decompress_chunk(v["bytes"])
            assert "unsupported" in str(ex.value), v["name"]
            with pytest.raises(Exception) as ex:
                blosc2.decompress_chunk_into(v["bytes"], bytearray(v["nbytes"]))
            assert "unsupported" in str(ex.value), v["name"]
        else:
            assert Z.sha(blosc2.decompress_chunk(v["bytes"])) == v["sha256"], v["name"]
    chunks = [v["bytes"] for v in vs]
    assert batch.blosc_chunk_sizes(chunks) == [-31 if r else v["nbytes"] for v, r in zip(vs, refused)]
    res, outs = batch.blosc_decompress_chunks(chunks)
    for v, r, got, o in zip(vs, refused, res, outs):
        assert got == (-31 if r else v["nbytes"]) and len(o) == (0 if r else v["nbytes"]), v["name"]
