"""DEFLATE batches on the GPU (cj_deflate_batch_* / cramjam_amd.batch.deflate_*): per wrapper every fixture, mutation and hand-written
stream of tests/deflate_cases.py through the device and the host entry, bad chunks between good ones, 64 guard bytes of 0xA5 around
every output slot; batches of 1, 3 and 5 chunks (idle wavefronts in the workgroup); the size query; capacities exact, exact - 1 and 0
against zlib's verdict at that capacity; a stream of more than 1 MiB; the argument checks; torch tensors on a side stream."""
import os

import numpy as np
import pytest

import deflate_cases as D
import device_batch as DB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _shuffled(wrap):
    cs = D.cases(wrap)
    return [cs[k] for k in np.random.default_rng(wrap + 1).permutation(len(cs))]      # bad chunks between good ones


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_device_batch_over_all_fixtures(eng, wrap):
    e, N = eng
    cs = _shuffled(wrap)
    assert sum(1 for c in cs if c["result"] < 0) >= 50 and sum(1 for c in cs if c["result"] >= 0) >= 50
    for part in (cs[:1], cs[1:4], cs[4:9], cs):                       # 1, 3 and 5 chunks: idle wavefronts in the last workgroup
        caps = [c["cap"] for c in part]
        res, out, ooff = D.device_call(e, N, wrap, [c["bytes"] for c in part], caps)
        for i, c in enumerate(part):
            assert res[i] == c["result"], (c["name"], int(res[i]), c["result"])
            if c["result"] >= 0:
                assert D.sha(out[ooff[i]:ooff[i] + c["result"]]) == c["sha256"], c["name"]
        assert DB.guards_intact(out, ooff, caps) is None


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_host_batch_over_all_fixtures(wrap):
    from cramjam_amd import batch
    cs = _shuffled(wrap)
    for part in (cs[:1], cs[1:4], cs[4:9], cs):
        chunks, caps = [c["bytes"] for c in part], [c["cap"] for c in part]
        res, outs = batch.deflate_decompress_many(chunks, output_lens=caps, wrapper=D.WRAP_NAME[wrap])
        for c, r, o in zip(part, res, outs):
            assert r == c["result"] and len(o) == max(r, 0) and (r < 0 or D.sha(o) == c["sha256"]), (c["name"], r)
    caps = [c["cap"] for c in cs[:40]]                                # ... into one caller's buffer
    buf = bytearray(b"\xa5" * (sum(caps) + 16))
    res2, views = batch.deflate_decompress_many([c["bytes"] for c in cs[:40]], output_lens=caps, wrapper=D.WRAP_NAME[wrap], out=buf)
    assert list(res2) == [c["result"] for c in cs[:40]] and all(D.sha(v) == c["sha256"] for v, c in zip(views, cs[:40]) if c["result"] >= 0)
    assert bytes(buf[sum(caps):]) == b"\xa5" * 16


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_size_query_and_the_decode_laid_out_from_it(eng, wrap):
    e, N = eng
    from cramjam_amd import batch
    cs = _shuffled(wrap)
    chunks = [c["bytes"] for c in cs]
    want = [D.size_verdict(wrap, s) for s in chunks]
    assert batch.deflate_sizes(chunks, wrapper=D.WRAP_NAME[wrap]) == want
    res, _, _ = D.device_call(e, N, wrap, chunks, [0] * len(cs), sizes=True)
    assert [int(r) for r in res] == want
    # the size query's errors are the decoder's, except checksum errors
    full = [D.verdict(wrap, s, None)[0] for s in chunks]
    assert all(w == f or f == D.CHECKSUM for w, f in zip(want, full))
    # without output_lens: through the query
    res, outs = batch.deflate_decompress_many(chunks, wrapper=D.WRAP_NAME[wrap])
    for c, s, f, r, o in zip(cs, want, full, res, outs):
        if s < 0:
            assert r == s and len(o) == 0, c["name"]
        else:
            assert r == f and (r < 0 or D.verdict(wrap, c["bytes"], None)[1] == bytes(o)), (c["name"], r, f)


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_capacities_exact_one_less_and_zero(eng, wrap):
    """zlib's verdict at that capacity, live; nothing outside a slot"""
    e, N = eng
    cs = [c for c in _shuffled(wrap) if c["name"] not in D.DIVERGES_FROM_ZLIB]
    chunks = [c["bytes"] for c in cs]
    exact = [c["result"] if c["result"] >= 0 else c["cap"] for c in cs]
    for caps in (exact, [max(x - 1, 0) for x in exact], [0] * len(cs)):
        res, out, ooff = D.device_call(e, N, wrap, chunks, caps)
        for i, c in enumerate(cs):
            r, raw = D.verdict(wrap, c["bytes"], caps[i])
            assert res[i] == r, (c["name"], caps[i], int(res[i]), r)
            assert r < 0 or out[ooff[i]:ooff[i] + r].tobytes() == raw, (c["name"], caps[i])
        assert DB.guards_intact(out, ooff, caps) is None


def test_a_stream_of_more_than_1_mib(eng):
    e, N = eng
    from cramjam_amd import batch
    t = D.flush_text()
    raw = b"".join(t[k:] + t[:k] for k in (0, 1111, 77777, 150001))           # 1.2 MB
    assert len(raw) > 1 << 20
    for wrap in D.WRAPS:
        s = D.compress(raw, 6, 0, wrap)
        res, out, ooff = D.device_call(e, N, wrap, [s, s[:len(s) // 2], s], [len(raw), len(raw), len(raw) - 1])
        assert list(res) == [len(raw), D.EOF, D.OUT_TOO_SMALL] and out[ooff[0]:ooff[0] + len(raw)].tobytes() == raw
        assert DB.guards_intact(out, ooff, [len(raw), len(raw), len(raw) - 1]) is None
        assert batch.deflate_sizes([s], wrapper=D.WRAP_NAME[wrap]) == [len(raw)]


def test_empty_batches_and_bad_arguments(eng):
    e, N = eng
    L = N.lib()
    from cramjam_amd import batch
    p = e.alloc(64)
    try:
        for wrap in D.WRAPS:
            assert L.cj_deflate_batch_device(e.h, wrap, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None, None, None, None) == 0
            assert L.cj_deflate_batch_sizes_device(e.h, wrap, 0, 0, None, None, None, None, None) == 0
            assert L.cj_deflate_batch_device(e.h, wrap, N.OP_COMPRESS, 0, 1, p, p, p, p, p, p, p, None) == D.BAD_ARG
            assert L.cj_deflate_batch_device(e.h, wrap, N.OP_DECOMPRESS, 1, 1, p, p, p, p, p, p, p, None) == D.BAD_ARG
            assert L.cj_deflate_batch_device(e.h, wrap, N.OP_DECOMPRESS, 0, 1, p, p, p, None, p, p, p, None) == D.BAD_ARG
            assert L.cj_deflate_batch_sizes_device(e.h, wrap, 4, 1, p, p, p, p, None) == D.BAD_ARG
            assert L.cj_deflate_batch_sizes_device(e.h, wrap, 0, 1, p, p, p, None, None) == D.BAD_ARG
            assert batch.deflate_decompress_many([], wrapper=D.WRAP_NAME[wrap]) in (([], []), ((), ()), ([], ()))
            assert batch.deflate_sizes([], wrapper=D.WRAP_NAME[wrap]) == []
        assert L.cj_deflate_batch_device(e.h, 3, N.OP_DECOMPRESS, 0, 1, p, p, p, p, p, p, p, None) == D.BAD_ARG
        assert L.cj_deflate_batch_sizes_device(e.h, 7, 0, 1, p, p, p, p, None) == D.BAD_ARG
    finally:
        e.free(p)
    # limits that belong to a chunk land in that chunk's result
    res, _ = batch.deflate_decompress_many([b"\x03\x00"], output_lens=[0], wrapper="raw")
    assert list(res) == [0]


def test_device_entries_on_torch_tensors_on_a_side_stream():
    """the device-resident calls on torch tensors with sync=False, in a child that imports torch BEFORE cramjam_amd (tests/device_api_child.py says why)"""
    DB.run_child(os.path.join(D.ROOT, "tests", "deflate_torch_child.py"), "deflate: ok", 600)
