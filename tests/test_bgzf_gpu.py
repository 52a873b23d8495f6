"""BGZF batches on the GPU (cj_bgzf_batch_* / cj_bgzf_sizes_* / cramjam_amd.batch.bgzf_*), against the model of
tests/bgzf_model.py: every case decoded as one host batch; a device batch of 1 000 streams, every third one malformed, with 64
canary bytes around every output slot; the size query; what the encoder writes — read back by gzip and by the decoder, its members
pinned to the DEFLATE encoder's bytes; capacities, turns of a shrunken slot budget, two engines, the `out=` form; torch tensors."""
import gzip
import os
import struct

import numpy as np
import pytest

import bgzf_model as M
import deflate_cases as D
import device_batch as DB

pytestmark = pytest.mark.gpu
SLOT = 65312    # bytes of one member slot of the compress scratch (cj_debug_bgzf_slot_budget counts in these)
SIZES = (0, 1, 65279, 65280, 65281, 130560, 200001)


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _device_call(e, N, op, chunks, caps):
    """cj_bgzf_batch_device in the harness's guarded run (tests/device_batch.py): chunks at every misalignment, slot i at least G bytes
    behind slot i - 1's end, at every misalignment too, the output filled with 0xA5 first: (results, output, offsets)"""
    n, L = len(chunks), N.lib()
    return DB.run_chunks(e, lambda i, o, l, out, oo, oc, r: N.check(L.cj_bgzf_batch_device(e.h, 0, op, 0, n, i, o, l, out, oo, oc, r, None)), chunks, caps, out_mis=DB.out_mis)


# ---- decode -------------------------------------------------------------------------------------------------------------------------
def test_every_model_case_as_one_host_batch():
    from cramjam_amd import batch
    names = list(M.cases())
    streams = [M.cases()[k][1] for k in names]
    caps = [max(M.sizes(s), 0) for s in streams]
    res, outs = batch.bgzf_decompress_many(streams, output_lens=caps)
    for k, r, o in zip(names, res, outs):
        assert (r, bytes(o)) == M.want(k), (k, r, M.want(k)[0])


_thousand = None


def thousand():
    """1 000 streams of 1 to 5 members, every third one malformed: [(stream, capacity, model result, model bytes, refused before decode)]"""
    global _thousand
    if _thousand is not None:
        return _thousand
    g = D._lcg(20240)
    pool = []
    for i in range(48):
        piece = M._text(10 + (next(g) % 3000), 300 + i)
        pool.append(M.member(piece, (0, 1, 9)[i % 3]))
    out = []
    for i in range(1000):
        mem = [pool[next(g) % len(pool)] for _ in range(1 + next(g) % 5)]
        s = b"".join(mem) + (M.MARKER if next(g) % 2 else b"")
        cap = None
        if i % 3 == 2:
            kind, j = (i // 3) % 7, next(g) % len(mem)
            at = sum(len(m) for m in mem[:j])                                   # member j begins here
            if kind == 0:
                s = s[:len(s) - 1 - next(g) % 40]                               # cut short: the walk's EOF
            elif kind == 1:
                s += b"\x5a"                                                    # a byte of garbage behind the last member
            elif kind == 2:
                cap = M.sizes(s) - 1                                            # the ISIZE sum exceeds the capacity
            elif kind == 3:
                p = at + len(mem[j]) - 8
                s = M._patch(s, p, bytes([s[p] ^ 0x40]))                        # CRC32 of member j
            elif kind == 4:
                p = at + len(mem[j]) - 4
                s = M._patch(s, p, struct.pack("<I", struct.unpack_from("<I", s, p)[0] + (1 if i % 2 else -1)))      # ISIZE +- 1
            elif kind == 5:
                s = M._patch(s, at + 1, b"\x8c")                                # bad magic in member j
            else:
                p = at + 18 + (next(g) % 8)
                s = M._patch(s, p, bytes([s[p] ^ 0x04]))                        # a bit inside the DEFLATE data
        size = M.sizes(s)
        if cap is None:
            cap = size if size >= 0 else 100 + i % 900
        r, o = M.decode(s, cap)
        out.append((s, cap, r, o, size < 0 or size > cap))
    assert sum(1 for x in out if x[2] < 0) > 250 and sum(1 for x in out if x[4]) > 100
    _thousand = out
    return out


def test_device_batch_of_a_thousand_streams_with_canaries(eng):
    e, N = eng
    rows = thousand()
    caps = [x[1] for x in rows]
    res, out, ooff = _device_call(e, N, N.OP_DECOMPRESS, [x[0] for x in rows], caps)
    for i, (s, cap, r, o, refused) in enumerate(rows):
        assert res[i] == r, (i, int(res[i]), r)
        if r >= 0:
            assert out[ooff[i]:ooff[i] + r].tobytes() == o, i
        if refused:                     # by the walk or for its capacity: the whole slot is untouched
            assert (out[ooff[i]:ooff[i] + cap] == 0xA5).all(), i
    assert DB.guards_intact(out, ooff, caps) is None


def test_sizes_and_decode_without_output_lens():
    from cramjam_amd import batch
    names = list(M.cases())
    streams = [M.cases()[k][1] for k in names]
    sizes = batch.bgzf_sizes(streams)
    assert list(sizes) == [M.sizes(s) for s in streams]
    res, outs = batch.bgzf_decompress_many(streams)
    res2, outs2 = batch.bgzf_decompress_many(streams, output_lens=[max(x, 0) for x in sizes])
    assert list(res) == list(res2) == [M.want(k)[0] for k in names]
    assert [bytes(o) for o in outs] == [bytes(o) for o in outs2] == [M.want(k)[1] for k in names]
    assert batch.bgzf_sizes([]) == [] and batch.bgzf_decompress_many([]) == ([], [])


# ---- encode -------------------------------------------------------------------------------------------------------------------------
_bufs = None


def buffers():
    """compressible and incompressible buffers of every size of SIZES"""
    global _bufs
    if _bufs is None:
        rnd = np.random.default_rng(7).integers(0, 256, max(SIZES), dtype=np.uint8).tobytes()
        text = D.words(max(SIZES), 77)
        _bufs = [text[:n] for n in SIZES] + [rnd[:n] for n in SIZES]
    return _bufs


_encoded = None


def encoded():
    """(results, streams) of bgzf_compress_many over buffers(), computed once"""
    global _encoded
    if _encoded is None:
        from cramjam_amd import batch
        res, outs = batch.bgzf_compress_many(buffers())
        _encoded = list(res), [bytes(o) for o in outs]
    return _encoded


def test_encoded_streams_read_back_and_have_the_structure():
    from cramjam_amd import batch
    bufs = buffers()
    res, outs = encoded()
    pieces, where = [], []
    for b, r, s in zip(bufs, res, outs):
        n = len(b)
        assert r == len(s) and 0 < r <= batch.bgzf_compress_bound(n), (n, r)
        assert gzip.decompress(s) == b, n
        code, mem = M.walk(s)
        assert code == 0 and len(mem) == (n + M.PIECE - 1) // M.PIECE + 1, n
        assert all(ln <= 65536 and isize <= M.PIECE for _, ln, isize in mem)
        assert s[mem[-1][0]:] == M.MARKER                                       # the marker last
        for k, (off, ln, isize) in enumerate(mem[:-1]):
            assert s[off:off + 16] == M.MARKER[:16] and isize == min(M.PIECE, n - k * M.PIECE), (n, k)
            pieces.append(b[k * M.PIECE:k * M.PIECE + isize])
            where.append(s[off + 18:off + ln - 8])
    back, raw = batch.bgzf_decompress_many(outs, output_lens=[len(b) for b in bufs])
    assert list(back) == [len(b) for b in bufs] and [bytes(x) for x in raw] == bufs
    # the DEFLATE payload of every member is the existing encoder's for that piece
    rres, routs = batch.deflate_compress_many(pieces, wrapper="raw")
    assert [bytes(o) for o in routs] == where and all(r > 0 for r in rres)
    # the incompressible full piece is one stored block: the largest member there is
    i = len(SIZES) + SIZES.index(65280)
    assert M.walk(outs[i])[1][0][1] == 65311 and res[i] == 65311 + 28


def test_capacities_bound_exact_and_one_less(eng):
    e, N = eng
    bufs = buffers()
    res, outs = encoded()
    L = N.lib()
    bound = [L.cj_bgzf_compress_bound(len(b)) for b in bufs]
    for caps in (bound, list(res), [r - 1 for r in res], [r - (i % 2) for i, r in enumerate(res)]):
        got, out, ooff = _device_call(e, N, N.OP_COMPRESS, bufs, caps)
        for i, s in enumerate(outs):
            if caps[i] >= res[i]:
                assert got[i] == res[i] and out[ooff[i]:ooff[i] + res[i]].tobytes() == s, (i, caps[i], int(got[i]))
            else:
                assert got[i] == M.OUT_TOO_SMALL and (out[ooff[i]:ooff[i] + caps[i]] == 0xA5).all(), (i, caps[i], int(got[i]))
        assert DB.guards_intact(out, ooff, caps) is None


def test_streams_across_turns_at_capacities_below_the_bound(eng):
    """two slots per turn: the buffers of three and four pieces span turns; below the bound such a stream is sized in a first pass and
    written in a second, or not at all"""
    e, N = eng
    bufs = [b for b in buffers() if len(b) >= 65281]
    res, outs = encoded()
    want = [(r, s) for b, r, s in zip(buffers(), res, outs) if len(b) >= 65281]
    L = N.lib()
    prev = L.cj_debug_bgzf_slot_budget(2 * SLOT)
    try:
        for caps in ([r for r, _ in want], [r - 1 for r, _ in want], [r - (i % 2) for i, (r, _) in enumerate(want)]):
            got, out, ooff = _device_call(e, N, N.OP_COMPRESS, bufs, caps)
            for i, (r, s) in enumerate(want):
                if caps[i] >= r:
                    assert got[i] == r and out[ooff[i]:ooff[i] + r].tobytes() == s, (i, caps[i], int(got[i]))
                else:
                    assert got[i] == M.OUT_TOO_SMALL and (out[ooff[i]:ooff[i] + caps[i]] == 0xA5).all(), (i, caps[i], int(got[i]))
            assert DB.guards_intact(out, ooff, caps) is None
    finally:
        assert L.cj_debug_bgzf_slot_budget(prev) == 2 * SLOT


def test_mixed_batch_of_500_buffers_through_three_turns_two_engines_and_out(eng):
    from cramjam_amd import batch
    e, N = eng
    L = N.lib()
    g = D._lcg(500)
    text, rnd = D.words(200000, 78), buffers()[-1]
    bufs = []
    for i in range(500):
        n = (0, 1, 700, 5000, 65280, 65281, 140000)[next(g) % 7] + (next(g) % 300 if i % 5 else 0)
        src = rnd if i % 4 == 3 else text
        at = next(g) % (len(src) - n)
        bufs.append(src[at:at + n])
    res, outs = batch.bgzf_compress_many(bufs)
    outs = [bytes(o) for o in outs]
    assert [gzip.decompress(s) for s in outs] == bufs and [len(s) for s in outs] == list(res)
    npieces = sum((len(b) + M.PIECE - 1) // M.PIECE for b in bufs)
    per = (npieces + 2) // 3
    assert (npieces + per - 1) // per == 3
    prev = L.cj_debug_bgzf_slot_budget(per * SLOT)                              # three turns
    try:
        res3, outs3 = batch.bgzf_compress_many(bufs)
    finally:
        assert L.cj_debug_bgzf_slot_budget(prev) == per * SLOT
    assert list(res3) == list(res) and [bytes(o) for o in outs3] == outs
    res2, outs2 = batch.bgzf_compress_many(bufs, devices=[0, 0])                # two host engines on device 0 equal one
    assert list(res2) == list(res) and [bytes(o) for o in outs2] == outs
    need = sum(batch.bgzf_compress_bound(len(b)) for b in bufs)
    buf = bytearray(b"\xa5" * (need + 16))
    res4, views = batch.bgzf_compress_many(bufs, out=buf)                       # the `out=` form equals the `bytes` form
    assert list(res4) == list(res) and [bytes(v) for v in views] == outs and bytes(buf[need:]) == b"\xa5" * 16
    back, raw = batch.bgzf_decompress_many(outs, devices=[0, 0])
    assert list(back) == [len(b) for b in bufs] and [bytes(x) for x in raw] == bufs


def test_an_input_above_the_limit_lands_in_its_own_result(eng):
    e, N = eng
    n = 3
    t = buffers()[2]
    d_in, d_out = e.alloc(len(t) + 64), e.alloc(3 * 70000)
    d_meta = [e.alloc(8 * n) for _ in range(5)]
    try:
        e.h2d(d_in, np.frombuffer(t, np.uint8))
        for p, a in zip(d_meta, ([0, 0, 0], [len(t), 0x7E000001, len(t)], [0, 70000, 140000], [70000] * 3)):
            e.h2d(p, np.array(a, np.uint64))
        N.check(N.lib().cj_bgzf_batch_device(e.h, 0, N.OP_COMPRESS, 0, n, d_in, d_meta[0], d_meta[1], d_out, d_meta[2], d_meta[3], d_meta[4], None))
        e.sync()
        res = e.d2h(d_meta[4], 8 * n, "int64")
        want = encoded()[0][2]
        assert [int(r) for r in res] == [want, M.INPUT_TOO_LARGE, want]
        assert e.d2h(d_out, 3 * 70000)[140000:140000 + want].tobytes() == encoded()[1][2]
    finally:
        for p in [d_in, d_out] + d_meta:
            e.free(p)


def test_device_entries_on_torch_tensors():
    """bgzf_compress_many_device, bgzf_sizes_device and bgzf_decompress_many_device on torch tensors on a side stream, in a child that
    imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(D.ROOT, "tests", "bgzf_torch_child.py"), "bgzf torch: ok", 600)
