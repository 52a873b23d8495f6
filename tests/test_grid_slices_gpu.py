"""The launch loop of the wavefront-per-chunk batches (cj::for_slices, cj::grid_chunks): with cj_debug_grid_chunks(5) a batch of 13
chunks goes through in launches that end at chunks 5, 10 and 13 — two full slices and a ragged one — and every entry point that
slices gives the same 13 results and the same bytes as in one launch.  An invalid chunk ends the first slice, an empty one begins the
last."""
import zlib

import numpy as np
import pytest

import device_batch as DB
import zstd_cases as Z

pytestmark = pytest.mark.gpu
N_CHUNKS, INVALID, EMPTY, SLICE = 13, 4, 10, 5


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _raws():
    rng = np.random.default_rng(18)
    words = [bytes(rng.integers(97, 123, 5, dtype=np.uint8)) for _ in range(24)]
    return [b" ".join(words[k] for k in rng.integers(0, 24, 40 + 5 * i)) for i in range(N_CHUNKS)]      # 240 .. 600 bytes each


def _run(e, N, chunks, caps, call):
    """call(n, d_in, in_off, in_len, d_out, out_off, out_cap, result) in the harness's guarded run (tests/device_batch.py): chunks at
    every misalignment, the output filled with 0xA5 first: (results, output, offsets)"""
    res, out, ooff = DB.run_chunks(e, lambda *a: N.check(call(len(chunks), *a)), chunks, caps)
    return [int(r) for r in res], out, ooff


def _both(e, N, chunks, caps, call):
    """the call in one launch and in slices of five: the same results and bytes; returns them"""
    res, out, ooff = _run(e, N, chunks, caps, call)
    prev = N.lib().cj_debug_grid_chunks(SLICE)
    try:
        res5, out5, _ = _run(e, N, chunks, caps, call)
    finally:
        assert N.lib().cj_debug_grid_chunks(prev) == SLICE
    assert res5 == res and (out5 == out).all()
    return res, [bytes(out[o:o + max(r, 0)]) for o, r in zip(ooff, res)]


def test_deflate_zlib_decode_and_sizes(eng):
    e, N = eng
    L = N.lib()
    raws = _raws()
    streams = [zlib.compress(r, 6) for r in raws]
    streams[INVALID] = streams[INVALID][:20] + bytes([streams[INVALID][20] ^ 0x40]) + streams[INVALID][21:-6]
    streams[EMPTY] = b""
    caps = [len(r) for r in raws]
    res, outs = _both(e, N, streams, caps, lambda n, i, io, il, o, oo, oc, r:
                      L.cj_deflate_batch_device(e.h, N.DEFLATE_ZLIB, N.OP_DECOMPRESS, 0, n, i, io, il, o, oo, oc, r, None))
    for k in range(N_CHUNKS):
        assert (res[k] < 0) if k in (INVALID, EMPTY) else (res[k] == len(raws[k]) and outs[k] == raws[k]), (k, res[k])
    sizes, _ = _both(e, N, streams, [0] * N_CHUNKS, lambda n, i, io, il, o, oo, oc, r:
                     L.cj_deflate_batch_sizes_device(e.h, N.DEFLATE_ZLIB, 0, n, i, io, il, r, None))
    assert [s for k, s in enumerate(sizes) if k not in (INVALID, EMPTY)] == [len(r) for k, r in enumerate(raws) if k not in (INVALID, EMPTY)]
    assert sizes[INVALID] < 0 and sizes[EMPTY] < 0


def test_zstd_decode_with_three_slots_and_sizes(eng):
    e, N = eng
    L = N.lib()
    cs = [c for c in Z.load_cases() if c.name not in Z.DIVERGES_FROM_ZSTD]
    good = [c for c in cs if c.accepted and 100 <= c.cap < 2048][:N_CHUNKS]
    bad = [c for c in cs if not c.accepted and c.cap < 2048][0]
    assert len(good) == N_CHUNKS
    streams, caps, want = [c.stream for c in good], [c.cap for c in good], [c.verdicts[0] for c in good]
    streams[INVALID], caps[INVALID], want[INVALID] = bad.stream, bad.cap, bad.verdicts[0]
    streams[EMPTY] = b""
    prev = L.cj_debug_zstd_slot_budget(3 * (131072 + 32))      # slices of three slots inside launches of at most five chunks
    try:
        res, outs = _both(e, N, streams, caps, lambda n, i, io, il, o, oo, oc, r:
                          L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, n, i, io, il, o, oo, oc, r, None))
    finally:
        assert L.cj_debug_zstd_slot_budget(prev) == 3 * (131072 + 32)
    # ... and with the default budget, where the slices of five are the only ones
    assert _both(e, N, streams, caps, lambda n, i, io, il, o, oo, oc, r:
                 L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, n, i, io, il, o, oo, oc, r, None)) == (res, outs)
    for k in range(N_CHUNKS):
        if k != EMPTY:
            assert res[k] == want[k] and (res[k] < 0 or Z.sha(np.frombuffer(outs[k], np.uint8)) == (bad if k == INVALID else good[k]).sha), (k, res[k])
    assert res[INVALID] < 0
    sizes, _ = _both(e, N, streams, [0] * N_CHUNKS, lambda n, i, io, il, o, oo, oc, r:
                     L.cj_zstd_batch_sizes_device(e.h, N.ZSTD_FRAMES, 0, n, i, io, il, r, None))
    assert all(sizes[k] == res[k] for k in range(N_CHUNKS) if k not in (INVALID, EMPTY))


def test_dictionary_compress_decode_and_sizes(eng):
    e, N = eng
    L = N.lib()
    raws = _raws()
    d = b" ".join(raws)[:3000]
    d_dict = e.alloc(len(d) + 32)
    try:
        e.h2d(d_dict, np.frombuffer(d, np.uint8))
        raws[EMPTY] = b""
        caps = [L.cj_lz4_block_compress_bound(len(r), 0) for r in raws]
        caps[INVALID] = 7                                          # too small: this chunk's compress fails
        compress = lambda n, i, io, il, o, oo, oc, r: L.cj_dict_batch_device(e.h, N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, 0, n, i, io, il, o, oo, oc, r, d_dict, len(d), None)  # noqa: E731
        cres, streams = _both(e, N, raws, caps, compress)
        # the staging budget cut to four slots (slices end at 4, 8, 12, 13): the same streams
        slot = (len(d) + 65536 + 255) & ~255
        prev = L.cj_debug_dict_stage_budget(4 * slot)
        try:
            assert _both(e, N, raws, caps, compress) == (cres, streams)
        finally:
            assert L.cj_debug_dict_stage_budget(prev) == 4 * slot
        # the prefix / verdict pass behind the encoder is one lane per chunk, its launches hold 64 times as many: 325 chunks make two of its slices of 5 * 64
        many = [raws[k % N_CHUNKS][:40 + k % 23] for k in range(325)]
        mcaps = [L.cj_lz4_block_compress_bound(len(r), 1) for r in many]
        mres, _ = _both(e, N, many, mcaps, lambda n, i, io, il, o, oo, oc, r:
                        L.cj_dict_batch_device(e.h, N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, N.FLAG_LZ4_SIZE_PREFIX, n, i, io, il, o, oo, oc, r, d_dict, len(d), None))
        assert all(r >= 4 for r in mres)
        assert cres[INVALID] < 0 and all(0 < cres[k] < len(raws[k]) for k in range(N_CHUNKS) if k not in (INVALID, EMPTY))
        streams[INVALID] = b"\xf0\xff\xff\xff"                    # a literal run whose length bytes run out
        streams[EMPTY] = b""
        res, outs = _both(e, N, streams, [len(r) for r in raws], lambda n, i, io, il, o, oo, oc, r:
                          L.cj_dict_batch_device(e.h, N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, 0, n, i, io, il, o, oo, oc, r, d_dict, len(d), None))
        sizes, _ = _both(e, N, streams, [0] * N_CHUNKS, lambda n, i, io, il, o, oo, oc, r:
                         L.cj_dict_batch_sizes_device(e.h, N.CODEC_LZ4_BLOCK, 0, n, i, io, il, r, len(d), None))
        for k in range(N_CHUNKS):
            if k in (INVALID, EMPTY):
                assert res[k] < 0 and sizes[k] < 0, (k, res[k], sizes[k])
            else:
                assert res[k] == sizes[k] == len(raws[k]) and outs[k] == raws[k], (k, res[k], sizes[k])
    finally:
        e.free(d_dict)
