"""LZ4 block batches against a shared dictionary on the GPU (cj_dict_batch_* / dictionary=...): every fixture, mutation and
hand-written stream of tests/lz4_dict_model.py through the device and the host entry, one batch per dictionary, with guard bytes around
every output slot; the empty dictionary against the plain call; the size query; the size prefix; the encoder against its scalar model
(tests/hostsim/enc2_linked_model.c with hist = dictionary), the chunk that is too long, the sliced staging, and what the dictionary
buys against liblz4 without one."""
import os

import numpy as np
import pytest

import device_batch as DB
import lz4_dict_model as D

pytestmark = pytest.mark.gpu
G = DB.G


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _device_call(e, N, op, flags, chunks, caps, d, plain=False):
    """cj_dict_batch_device (plain: cj_batch_device) in the harness's guarded run (tests/device_batch.py): chunks at every misalignment,
    the dictionary 3 bytes off a granule, G guard bytes around every slot, the output filled with 0xA5 first: (results, output, offsets)"""
    n, L = len(chunks), N.lib()
    if plain:
        call = lambda i, o, l, out, oo, oc, r, dd: N.check(L.cj_batch_device(e.h, 0, op, flags, n, i, o, l, out, oo, oc, r, None))
    else:
        call = lambda i, o, l, out, oo, oc, r, dd: N.check(L.cj_dict_batch_device(e.h, 0, op, flags, n, i, o, l, out, oo, oc, r, dd if len(d) else None, len(d), None))
    return DB.run_chunks(e, call, chunks, caps, dictionary=d)


def _guards_intact(out, ooff, caps, res, may_write_inside):
    """nothing outside the slots; inside a slot nothing behind the bytes produced (a refused chunk may have written inside its slot)"""
    bad = DB.first_dirty(out, DB.untouched(ooff, res, len(out), written=caps if may_write_inside else None), ooff)
    return None if bad is None else bad[0]


def test_device_batches_over_all_fixtures_one_batch_per_dictionary(eng):
    e, N = eng
    total = 0
    for dl in D.BATCH_DICT_LENS:
        cs = D.cases(dl)
        order = np.random.default_rng(dl).permutation(len(cs))       # bad chunks between good ones
        cs = [cs[k] for k in order]
        caps = [c["cap"] for c in cs]
        res, out, ooff = _device_call(e, N, N.OP_DECOMPRESS, 0, [c["bytes"] for c in cs], caps, D.dictionary(dl))
        for i, c in enumerate(cs):
            assert res[i] == c["result"], (dl, c["name"], int(res[i]), c["result"])
            if c["result"] >= 0:
                assert D.sha(out[ooff[i]:ooff[i] + c["result"]]) == c["sha256"], (dl, c["name"])
        assert _guards_intact(out, ooff, caps, res, True) is None, dl
        total += len(cs)
    assert total == len(D.valid()) + len(D.mutations()) + len(D.hand())
    assert sum(1 for dl in D.BATCH_DICT_LENS for c in D.cases(dl) if c["result"] < 0) >= 50


def test_host_batches_over_all_fixtures_one_batch_per_dictionary():
    from cramjam_amd import batch
    for dl in D.BATCH_DICT_LENS:
        cs = D.cases(dl)
        chunks, caps = [c["bytes"] for c in cs], [c["cap"] for c in cs]
        res, outs = batch.lz4_decompress_blocks(chunks, output_lens=caps, dictionary=D.dictionary(dl))
        for c, r, o in zip(cs, res, outs):
            assert r == c["result"] and len(o) == max(r, 0) and (r < 0 or D.sha(o) == c["sha256"]), (dl, c["name"], r)
        if dl == 4096:                                                # ... into one caller's buffer
            buf = bytearray(b"\xa5" * (sum(caps) + 16))
            res2, views = batch.lz4_decompress_blocks(chunks, output_lens=caps, dictionary=bytearray(D.dictionary(dl)), out=buf)
            assert list(res2) == list(res) and [bytes(v) for v in views] == [bytes(o) for o in outs]
            assert bytes(buf[sum(caps):]) == b"\xa5" * 16


def test_dictionary_of_length_0_is_the_plain_call(eng):
    e, N = eng
    from cramjam_amd import batch
    raws = [D.words(n, 40 + k) for k, n in enumerate((0, 1, 13, 300, 4096, 65536, 70000))]
    res, comp = batch.lz4_compress_blocks(raws, store_size=False)
    chunks = [bytes(c) for c in comp] + [h["bytes"] for h in D.hand()]       # ... and streams that need a dictionary: refused by both
    caps = [len(r) for r in raws] + [h["cap"] for h in D.hand()]
    for flags in (0, N.FLAG_LZ4_SIZE_PREFIX):
        a = _device_call(e, N, N.OP_DECOMPRESS, flags, chunks, caps, b"")
        b = _device_call(e, N, N.OP_DECOMPRESS, flags, chunks, caps, b"", plain=True)
        assert list(a[0]) == list(b[0])
        for i, lo in enumerate(a[2]):                                 # (what a refused chunk left inside its slot is not compared)
            used = max(int(a[0][i]), 0)
            assert (a[1][lo - G:lo + used] == b[1][lo - G:lo + used]).all() and (a[1][lo + caps[i]:lo + caps[i] + G] == 0xA5).all(), i
        bounds = [N.lib().cj_lz4_block_compress_bound(len(r), 1) for r in raws]
        a = _device_call(e, N, N.OP_COMPRESS, flags, raws, bounds, b"")
        b = _device_call(e, N, N.OP_COMPRESS, flags, raws, bounds, b"", plain=True)
        assert list(a[0]) == list(b[0]) and (a[1] == b[1]).all() and all(r > 0 for r in a[0])
    assert sum(1 for r in _device_call(e, N, N.OP_DECOMPRESS, 0, chunks, caps, b"")[0] if r == D.CORRUPT) >= 10
    for store in (False, True):
        p, q = batch.lz4_compress_blocks(raws, store_size=store, dictionary=b""), batch.lz4_compress_blocks(raws, store_size=store)
        assert list(p[0]) == list(q[0]) and [bytes(x) for x in p[1]] == [bytes(x) for x in q[1]]
    p = batch.lz4_decompress_blocks(chunks, output_lens=caps)
    q = batch.lz4_decompress_blocks(chunks, output_lens=caps, dictionary=b"")
    assert list(p[0]) == list(q[0]) and [bytes(x) for x in p[1]] == [bytes(x) for x in q[1]]
    assert batch.lz4_block_sizes(chunks, dictionary=b"") == batch.lz4_block_sizes(chunks)
    p, q = batch.lz4_decompress_blocks(chunks), batch.lz4_decompress_blocks(chunks, dictionary=b"")
    assert list(p[0]) == list(q[0]) and [bytes(x) for x in p[1]] == [bytes(x) for x in q[1]]


def test_size_query_is_exact_and_a_decode_laid_out_from_it_succeeds():
    from cramjam_amd import batch
    for dl in D.BATCH_DICT_LENS:
        cs = D.cases(dl)
        chunks = [c["bytes"] for c in cs]
        sizes = batch.lz4_block_sizes(chunks, dictionary=D.dictionary(dl))
        assert sizes == [D.size_walk(s, dl) for s in chunks], dl
        res, outs = batch.lz4_decompress_blocks(chunks, dictionary=D.dictionary(dl))            # no output_lens: through the query
        for c, s, r, o in zip(cs, sizes, res, outs):
            if s < 0:
                assert r == s and len(o) == 0, c["name"]
            elif c["result"] == s:                                    # an intact stream (or a mutation that kept its size)
                assert r == s and D.sha(o) == c["sha256"], (dl, c["name"], r)
            else:                                                     # whatever the model says at exactly that capacity
                assert r == D.decode(c["bytes"], s, D.dictionary(dl))[0], (dl, c["name"], r)
    # without the dictionary's length the walk refuses the streams that need it
    need = [v["bytes"] for v in D.valid() if v["dict_len"] == 65536 and v["n"] >= 300]
    assert all(s == D.CORRUPT for s in batch.lz4_block_sizes(need))


def test_size_prefix_in_both_directions(eng):
    e, N = eng
    from cramjam_amd import batch
    d = D.dictionary(4096)
    cs = D.cases(4096)
    pre = [c["cap"].to_bytes(4, "little") + c["bytes"] for c in cs]
    caps = [c["cap"] + 7 for c in cs]                                 # the prefix, not the capacity, bounds the decode
    res, out, ooff = _device_call(e, N, N.OP_DECOMPRESS, N.FLAG_LZ4_SIZE_PREFIX, pre, caps, d)
    for i, c in enumerate(cs):
        assert res[i] == c["result"] and (c["result"] < 0 or D.sha(out[ooff[i]:ooff[i] + c["result"]]) == c["sha256"]), c["name"]
    assert _guards_intact(out, ooff, caps, res, True) is None
    assert batch.lz4_block_sizes(pre, store_size=True, dictionary=d) == [c["cap"] for c in cs]
    short = [p[:3] for p in pre[:4]] + [b"\xff\xff\xff\xff" + pre[0][4:], (caps[1] + 1).to_bytes(4, "little") + pre[1][4:]]
    res, outs = batch.lz4_decompress_blocks(short, output_lens=caps[:4] + [caps[0], caps[1]], store_size=True, dictionary=d)
    assert list(res) == [D.NO_PREFIX] * 4 + [D.NEG_PREFIX, D.OUT_TOO_SMALL]
    raws = [D.words(n, 70 + k) for k, n in enumerate((0, 5, 300, 4096, 65536))]
    res, comp = batch.lz4_compress_blocks(raws, dictionary=d)          # store_size=True is the default
    assert all(int.from_bytes(c[:4], "little") == len(r) and rr == len(c) for c, r, rr in zip(comp, raws, res))
    res, outs = batch.lz4_decompress_blocks(comp, store_size=True, dictionary=d)
    assert list(res) == [len(r) for r in raws] and [bytes(o) for o in outs] == raws


def _records():
    """word-like records of the dictionary's vocabulary, two per size class"""
    return [D.words(n, 500 + 10 * k + j) for k, n in enumerate((0, 1, 12, 13, 64, 300, 4096, 16384, 65535, 65536)) for j in range(2)]


def test_compress_equals_the_encoder_model_and_decodes_everywhere(eng):
    e, N = eng
    from cramjam_amd import batch
    from test_enc2_linked_model import linked_lib, model_linked
    M, L = linked_lib(), D.liblz4()
    raws = _records()
    bounds = [N.lib().cj_lz4_block_compress_bound(len(r), 0) for r in raws]
    for dl in (1, 7, 4096, 65535, 65536, 70000):
        d = D.dictionary(dl)
        want = [model_linked(M, d, r) for r in raws]
        res, out, ooff = _device_call(e, N, N.OP_COMPRESS, 0, raws, bounds, d)
        got = [out[ooff[i]:ooff[i] + max(int(res[i]), 0)].tobytes() for i in range(len(raws))]
        assert [int(r) for r in res] == [len(w) for w in want] and got == want, dl
        assert _guards_intact(out, ooff, bounds, res, False) is None, dl
        hres, hcomp = batch.lz4_compress_blocks(raws, store_size=False, dictionary=d)
        assert list(hres) == [len(w) for w in want] and [bytes(c) for c in hcomp] == want, dl
        # ... every output decodes to its input through the GPU's dictionary decoder, and through liblz4
        dres, douts = batch.lz4_decompress_blocks(got, output_lens=[len(r) for r in raws], dictionary=d)
        assert list(dres) == [len(r) for r in raws] and [bytes(o) for o in douts] == raws, dl
        if L is not None:
            for s, r in zip(got, raws):
                assert D.lz4_decode_using_dict(L, s, len(r), d) == (len(r), r), (dl, len(r))


def test_a_chunk_above_64k_is_refused_alone(eng):
    e, N = eng
    from cramjam_amd import batch
    d = D.dictionary(65536)
    raws = [D.words(4096, 1), D.words(65537, 2), D.words(65536, 3), D.words(200000, 4), D.words(13, 5)]
    alone = batch.lz4_compress_blocks([raws[0], raws[2], raws[4]], store_size=False, dictionary=d)
    for store in (False, True):
        res, comp = batch.lz4_compress_blocks(raws, store_size=store, dictionary=d)
        assert res[1] == D.INPUT_TOO_LARGE and res[3] == D.INPUT_TOO_LARGE and len(comp[1]) == 0 and len(comp[3]) == 0
        pre = 4 if store else 0
        assert [bytes(comp[i])[pre:] for i in (0, 2, 4)] == [bytes(c) for c in alone[1]]
    bounds = [N.lib().cj_lz4_block_compress_bound(len(r), 1) for r in raws]
    res, out, ooff = _device_call(e, N, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, raws, bounds, d)
    assert [int(r) for r in res] == [len(alone[1][0]) + 4, D.INPUT_TOO_LARGE, len(alone[1][1]) + 4, D.INPUT_TOO_LARGE, len(alone[1][2]) + 4]
    assert _guards_intact(out, ooff, bounds, res, True) is None
    # a capacity below the bound is "Compression failed", as in the plain call
    res, out, ooff = _device_call(e, N, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, raws[:1] * 3, [bounds[0], bounds[0] - 1, 3], d)
    assert [int(r) for r in res] == [len(alone[1][0]) + 4, -2, -2] and _guards_intact(out, ooff, [bounds[0], bounds[0] - 1, 3], res, False) is None


def test_a_batch_of_more_than_one_staging_slice_equals_the_unsliced_result(eng):
    e, N = eng
    raws = _records()[4:] + [D.words(65537, 9)]
    bounds = [N.lib().cj_lz4_block_compress_bound(len(r), 1) for r in raws]
    d = D.dictionary(70000)
    whole = _device_call(e, N, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, raws, bounds, d)
    prev = N.lib().cj_debug_dict_stage_budget(3 * 131072 + 5)         # three slots of `64 KiB of dictionary | 64 KiB of chunk` per slice
    try:
        assert prev == 1 << 30
        sliced = _device_call(e, N, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, raws, bounds, d)
        N.lib().cj_debug_dict_stage_budget(1)                         # below one slot: one chunk per slice
        single = _device_call(e, N, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, raws, bounds, d)
    finally:
        N.lib().cj_debug_dict_stage_budget(0)
    assert len(raws) > 2 * 3
    for other in (sliced, single):
        assert list(other[0]) == list(whole[0]) and (other[1] == whole[1]).all()
    assert whole[0][-1] == D.INPUT_TOO_LARGE and all(r > 4 for r in whole[0][:-1])


def test_the_dictionary_beats_liblz4_without_one_in_every_size_class():
    """the gate: per record-size class of 256 bytes and more, the GPU's total WITH the dictionary is smaller than liblz4's total
    WITHOUT one.  The ratio against liblz4 with the dictionary is printed, not gated (DESIGN.md 5.11 records it)."""
    from cramjam_amd import batch
    L = D.liblz4()
    d = D.dictionary(65536)
    for size in (300, 4096, 16384, 65536):
        raws = [D.words(size, 7000 + size + k) for k in range(16)]
        res, comp = batch.lz4_compress_blocks(raws, store_size=False, dictionary=d)
        gpu = sum(res)
        if L is not None:
            plain = sum(len(D.lz4_compress_plain(L, r)) for r in raws)
            with_dict = sum(len(D.lz4_compress_with_dict(L, r, d)) for r in raws)
            print("size %6d: gpu with dictionary %7d  liblz4 without %7d  liblz4 with %7d  gpu / liblz4-with %.3f" % (size, gpu, plain, with_dict, gpu / with_dict))
        else:
            import oracle
            plain = sum(oracle.lz4_compress_raw(r)[0] for r in raws)
        assert all(r > 0 for r in res) and gpu < plain, (size, gpu, plain)


def test_device_entries_on_torch_tensors_on_a_side_stream():
    """the device-resident calls with dictionary=<tensor>, in a child that imports torch BEFORE cramjam_amd (tests/device_api_child.py says why)"""
    DB.run_child(os.path.join(D.ROOT, "tests", "lz4_dict_torch_child.py"), "dictionary: ok", 600)
