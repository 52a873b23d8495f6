"""Blosc chunks on the GPU: the fixtures c-blosc minted through every decode entry, malformed chunks between intact neighbours, the
filter kernels alone against the model, and this library's own chunks through the model decoder (and c-blosc where it loads)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import blosc_cases as K
import blosc_model as M
import device_batch as DB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def test_fixtures_single_chunk():
    from cramjam_amd import blosc2
    for v in K.valid():
        out = blosc2.decompress_chunk(v["bytes"])
        assert len(out) == v["nbytes"] and K.sha(out) == v["sha256"], v["name"]
    for v in K.valid()[::7]:
        buf = bytearray(v["nbytes"] + 5)
        assert blosc2.decompress_chunk_into(v["bytes"], buf) == v["nbytes"] and K.sha(buf[:v["nbytes"]]) == v["sha256"], v["name"]
        assert bytes(buf[v["nbytes"]:]) == bytes(5)
    for v in K.valid(supported=False):
        with pytest.raises(Exception) as e:
            blosc2.decompress_chunk(v["bytes"])
        assert "unsupported" in str(e.value), v["name"]


def test_fixtures_host_batch_one_call():
    from cramjam_amd import batch
    vs = K.valid()
    order = np.random.default_rng(3).permutation(len(vs))
    chunks = [vs[i]["bytes"] for i in order]
    sizes = batch.blosc_chunk_sizes(chunks)
    assert sizes == [vs[i]["nbytes"] for i in order]
    res, outs = batch.blosc_decompress_chunks(chunks)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] and K.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]
    buf = bytearray(sum(sizes))
    res, outs = batch.blosc_decompress_chunks(chunks, out=buf)
    for k, i in enumerate(order):
        assert res[k] == vs[i]["nbytes"] and K.sha(outs[k]) == vs[i]["sha256"], vs[i]["name"]


def _torch_child(what):
    """the checks on torch tensors run in a child that imports torch BEFORE cramjam_amd (tests/device_api_child.py says why)"""
    DB.run_child(os.path.join(K.ROOT, "tests", "blosc_torch_child.py"), what + ": ok", 900, what)


def test_fixtures_device_batch_on_a_side_stream():
    _torch_child("fixtures")


def test_malformed_chunks_between_intact_neighbours(eng):
    e, N = eng
    good = [v for v in K.valid() if 4000 <= v["nbytes"] <= 70000][:2]
    bad = K.malformed()
    chunks, expect = [], []
    CAP = 300016                                                    # above every base chunk's nbytes: the verdicts are the fixtures' own
    for m in bad:
        cls, out = M.verdict(m["bytes"], CAP)
        assert cls == m["verdict"], m["name"]
        chunks += [good[0]["bytes"], m["bytes"], good[1]["bytes"]]
        expect += [("ok", good[0]), (cls, m), ("ok", good[1])]
    blob, off, ln = K.pack(chunks)
    G = 64
    caps = np.array([(x["nbytes"] if "recipe" in x else CAP) for cls, x in expect], np.uint64)
    slots = (caps + 15) // 16 * 16 + 2 * G
    ooff = (np.concatenate([[0], np.cumsum(slots)[:-1]]) + G).astype(np.uint64)
    total = int(slots.sum())
    call = lambda i, o, l, out, oo, oc, r: N.check(N.lib().cj_blosc_batch_device(e.h, 0, i, o, l, out, oo, oc, r, len(chunks), None, 0, None))
    res, out = DB.run(e, call, blob, off, ln, ooff, caps, total)
    for i, (cls, x) in enumerate(expect):
        lo, cap = int(ooff[i]), int(caps[i])
        if cls == "ok":
            assert res[i] == x["nbytes"] and K.sha(out[lo:lo + x["nbytes"]]) == x["sha256"], (i, x["name"], res[i])
            used = x["nbytes"]
        else:
            assert res[i] == M.CODE[cls], (x["name"], res[i], cls)
            # refused from its header or for its size: nothing written; a bad LZ4 stream shows only after streams before it (and,
            # in blocks that need no transposition, its own start) were decoded into the slot: nothing outside the slot
            used = cap if cls == M.CORRUPT else 0
        assert (out[lo + used:lo + ((cap + 15) // 16 * 16) + G] == 0xA5).all() and (out[lo - G:lo] == 0xA5).all(), (i, x["name"])


def _filter(e, N, forward, filt, ts, data, src_mis=0, dst_mis=0):
    n = len(data)
    d_src, d_dst = e.alloc(n + 64), e.alloc(n + 64)
    N.check(N.lib().cj_memset_dev(e.h, d_dst, 0x5A, n + 64))
    if n:
        N.check(N.lib().cj_memcpy_h2d(e.h, d_src + src_mis, np.frombuffer(data, np.uint8).ctypes.data, n))
    N.check(N.lib().cj_debug_blosc_filter(e.h, forward, filt, ts, d_src + src_mis, d_dst + dst_mis, n, 0, 1, None))
    out = e.d2h(d_dst, n + 64)
    e.free(d_src); e.free(d_dst)
    assert (out[:dst_mis] == 0x5A).all() and (out[dst_mis + n:] == 0x5A).all(), "filter kernel wrote outside its block"
    return out[dst_mis:dst_mis + n].tobytes()


def test_filter_kernels_alone_against_the_model(eng):
    e, N = eng
    rng = np.random.default_rng(11)
    for ts in list(range(1, 34)) + [64, 255]:
        sizes = {0, 1, ts - 1, ts, 8 * ts - 1, 8 * ts, 8 * ts + 1, 16 * ts + 3, 64 * ts, 1000 * ts + (ts - 1)}
        if ts in (1, 2, 4, 7, 8, 16, 17, 255):
            sizes |= {8 * 5000 * ts, 8 * 5000 * ts + 5, 70001}
        for k, n in enumerate(sorted(s for s in sizes if s >= 0)):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            for filt in (1, 2):
                mode = M.block_mode(1 if filt == 1 else 4, ts, n)
                mis = ((k + filt) % 4, (k * 3 + ts) % 8)
                want = M.apply_filter(data, ts, mode, True)
                assert _filter(e, N, 1, filt, ts, data, *mis) == want, ("filter", ts, n, filt)
                assert _filter(e, N, 0, filt, ts, want, *mis) == data, ("unfilter", ts, n, filt)


def _libblosc():
    sys.path.insert(0, os.path.join(K.ROOT, "tests", "golden"))
    import make_golden_blosc as G
    return G.load_libblosc()


def _check_own_chunk(chunk, raw, ts, lib):
    chunk = bytes(chunk)
    h, streams = M.parse(chunk)
    assert h["cbytes"] == len(chunk) and h["nbytes"] == len(raw) and h["typesize"] == ts and h["version"] == 2
    if not h["flags"] & 2 and len(raw):
        starts = [int.from_bytes(chunk[16 + 4 * b:20 + 4 * b], "little") for b in range(h["nblocks"])]
        assert starts == sorted(starts) and starts[0] == 16 + 4 * h["nblocks"]
        full = len(raw) // h["blocksize"]
        assert len(streams) == full * (1 if h["flags"] & 16 else ts) + (1 if len(raw) % h["blocksize"] else 0)
        assert all(s[3] <= 65536 for s in streams)
    assert M.decode(chunk) == raw
    if lib is not None:
        n = C.c_size_t(0)
        assert lib.blosc_cbuffer_validate(chunk, len(chunk), C.byref(n)) == 0 and n.value == len(raw)
        out = C.create_string_buffer(max(len(raw), 1))
        assert lib.blosc_decompress_ctx(chunk, out, len(raw), 1) == len(raw) and out.raw[:len(raw)] == raw


KINDS = ["f32", "text", "rand", "zeros", "i16", "f64"]
SIZES = [1, 31, 32, 100, 4095, 65536, 65537, 262144, 300001, 1 << 20, 1 << 23]


def _compress_inputs(ts, filt):
    """every size from 1 byte to 8 MiB with the data kinds rotating along them, and every kind at 300 001 bytes (a leftover block)"""
    bufs = [M.make_input(KINDS[(k + ts + filt) % 6], size, 1000 + k) for k, size in enumerate(SIZES)]
    return bufs + [M.make_input(kind, 300001, 2000 + k) for k, kind in enumerate(KINDS)]


def _compress_on_device(e, N, bufs, ts, filt, clevel, codec):
    """cj_blosc_batch_device(op = compress) on chunks that lie in HBM at odd offsets: (results, chunks), guard bytes checked"""
    blob, off, ln = K.pack(bufs)
    off = off + 1                                                   # (unaligned inputs)
    blob = np.concatenate([np.zeros(1, np.uint8), blob])
    G = 32
    caps = (ln + 32).astype(np.uint64)
    slots = (caps + 15) // 16 * 16 + 2 * G
    ooff = (np.concatenate([[0], np.cumsum(slots)[:-1]]) + G).astype(np.uint64)
    total = int(slots.sum())
    params = N.BloscParams(ts, filt, clevel, codec, 0)
    call = lambda i, o, l, out, oo, oc, r: N.check(N.lib().cj_blosc_batch_device(e.h, 1, i, o, l, out, oo, oc, r, len(bufs), C.byref(params), 0, None))
    res, out = DB.run(e, call, blob, off, ln, ooff, caps, total)
    chunks = []
    for i in range(len(bufs)):
        lo, r = int(ooff[i]), int(res[i])
        assert r > 0, (ts, filt, len(bufs[i]), r)
        assert (out[lo - G:lo] == 0xA5).all() and (out[lo + r:lo + int(slots[i]) - G] == 0xA5).all(), (ts, filt, len(bufs[i]))
        chunks.append(out[lo:lo + r].tobytes())
    return res, chunks


def test_compress_chunks_decode_with_the_model_and_c_blosc(eng):
    from cramjam_amd import batch, blosc2
    e, N = eng
    lib = _libblosc()
    print("c-blosc leg:", "ran" if lib is not None else "did not run (libblosc.so.1 is not installed here)")
    for ts in (1, 2, 4, 8, 16, 17):
        for filt in (0, 1, 2):
            bufs = _compress_inputs(ts, filt)
            clevel, codec = (5 if ts != 16 else 9), (1 if ts != 8 else 2)
            res, outs = batch.blosc_compress_chunks(bufs, ts, filter=filt, clevel=clevel, codec=codec)      # host batch
            for r, o, raw in zip(res, outs, bufs):
                assert r == len(o) <= len(raw) + 16, (ts, filt, len(raw), r)
                _check_own_chunk(o, raw, ts, lib)
            dres, douts = _compress_on_device(e, N, bufs, ts, filt, clevel, codec)                         # device-resident batch
            for r, o, h, raw in zip(dres, douts, outs, bufs):
                assert o == bytes(h), (ts, filt, len(raw))           # the same chunk from either entry (checked above)
            for raw, o in zip(bufs[:len(SIZES)], outs):                                                     # single chunk, every size
                one = blosc2.compress_chunk(raw, typesize=ts, clevel=blosc2.CLevel(clevel), filter=blosc2.Filter(filt), codec=blosc2.Codec(codec))
                assert bytes(one) == bytes(o), (ts, filt, len(raw))
                assert bytes(blosc2.decompress_chunk(one)) == raw
    # clevel 0: memcpyed; typesize from the buffer's itemsize; exact fit and one byte short
    a = np.arange(50000, dtype=np.float32)
    c0 = bytes(blosc2.compress_chunk(a, clevel=blosc2.CLevel.Zero))
    assert len(c0) == a.nbytes + 16 and c0[2] & 2 and c0[3] == 4 and M.decode(c0) == a.tobytes()
    c = bytes(blosc2.compress_chunk(a))
    assert c[3] == 4 and c[2] & 1 and len(c) < a.nbytes // 2 and M.decode(c) == a.tobytes()
    fit = bytearray(len(c))
    assert blosc2.compress_chunk_into(a, fit) == len(c) and bytes(fit) == c
    short = bytearray(b"\x77" * (len(c) - 1))
    with pytest.raises(Exception) as e:
        blosc2.compress_chunk_into(a, short)
    assert "Compression failed" in str(e.value) and bytes(short) == b"\x77" * (len(c) - 1)
    for bad in (dict(codec=blosc2.Codec.ZSTD), dict(codec=blosc2.Codec.BloscLz), dict(filter=blosc2.Filter.Delta)):
        with pytest.raises(Exception) as e:
            blosc2.compress_chunk(a, **bad)
        assert "unsupported" in str(e.value)


def test_round_trip_of_10000_chunks_device_resident():
    _torch_child("round_trip")


def test_capacities_empty_batch_and_single_chunk():
    from cramjam_amd import batch, blosc2
    v = next(x for x in K.valid() if x["nbytes"] == 70000 and x["recipe"]["filter"] == 1)
    raw = K.raw_of(v)
    assert batch.blosc_decompress_chunks([]) == ([], []) and batch.blosc_chunk_sizes([]) == []
    res, outs = batch.blosc_decompress_chunks([v["bytes"]])
    assert res == [70000] and bytes(outs[0]) == raw
    exact = bytearray(70000)
    assert blosc2.decompress_chunk_into(v["bytes"], exact) == 70000 and bytes(exact) == raw
    short = bytearray(b"\x11" * 69999)
    with pytest.raises(Exception) as e:
        blosc2.decompress_chunk_into(v["bytes"], short)
    assert "large enough" in str(e.value) and bytes(short) == b"\x11" * 69999
    big = bytearray(b"\x22" * 500000)
    assert blosc2.decompress_chunk_into(v["bytes"], big) == 70000 and bytes(big[:70000]) == raw and bytes(big[70000:]) == b"\x22" * 430000
