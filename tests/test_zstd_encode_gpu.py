"""Zstandard compress batches on the GPU (cj_zstd_compress_batch_* / cramjam_amd.batch.zstd_compress_*): with and
without the checksum flag the kernel's bytes against the scalar model's (tests/hostsim/zstd_enc_model.c) on every case of
tests/zstd_enc_cases.py, through the device and the C host entry, 64 guard bytes of 0xA5 around every output slot of both, inputs and
outputs at every misalignment; the same frames decoded on the device behind the encoder on the same stream without a wait in between,
and sized by the size query; capacities exact, exact - 1, 0 and mixed and batches of 1, 3 and 5 through both entries; a batch of 20
through seven turns at a shrunken slot budget; the argument checks; torch tensors on a side stream; two engines on one device.
Needs neither libzstd nor anything outside the repository."""
import os

import numpy as np
import pytest

import device_batch as DB
import zstd_enc_cases as E

pytestmark = pytest.mark.gpu
_want = {}


def want(name, flags):
    """(result, frame) of the model, computed once"""
    if (name, flags) not in _want:
        _want[(name, flags)] = E.model(E.cases()[name], flags)[:2]
    return _want[(name, flags)]


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _device_call(e, N, flags, chunks, caps, decode=False, in_lens=None):
    """cj_zstd_compress_batch_device in the harness's guarded run (tests/device_batch.py): chunks at every misalignment, slot i at least
    G bytes behind slot i - 1's end, at every misalignment too, the output filled with 0xA5 first: (results, output, offsets).
    decode: the frames are then sized by cj_zstd_batch_sizes_device and decoded by cj_zstd_batch_device on the same stream, with the
    encoder's device results as their in_len and no wait in between: (.., decoded results, decoded output, its offsets, sizes) are appended"""
    n, L = len(chunks), N.lib()
    blob, off, lens = DB.pack(chunks)
    ooff, total = DB.out_slots(caps, mis=DB.out_mis)
    with DB.device_batch(e, blob, off, lens if in_lens is None else in_lens, ooff, caps, total) as b:
        d_out, out_off, res = b.args[3], b.args[4], b.args[6]
        if decode:
            d_dec, dec_off, dec_cap, dres, doff, dtotal = b.output([len(c) for c in chunks])
            sizes = b.result_row()
        N.check(L.cj_zstd_compress_batch_device(e.h, N.ZSTD_FRAMES, flags, n, *b.args, None))
        if decode:          # in_len = the encoder's results, still on the device
            N.check(L.cj_zstd_batch_sizes_device(e.h, N.ZSTD_FRAMES, 0, n, d_out, out_off, res, sizes, None))
            N.check(L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, n, d_out, out_off, res, d_dec, dec_off, dec_cap, dres, None))
        got = b.read() + ([int(o) for o in ooff],)
        return got + (b.read_row(dres), e.d2h(d_dec, dtotal), doff, b.read_row(sizes)) if decode else got


@pytest.mark.parametrize("flags", E.FLAGS)
def test_device_batch_emits_the_models_bytes_and_the_decoder_reads_them(eng, flags):
    e, N = eng
    names = list(E.cases())
    chunks = [E.cases()[k] for k in names]
    caps = [E.bound(len(c), flags) for c in chunks]
    res, out, ooff, dres, dout, doff, sizes = _device_call(e, N, flags, chunks, caps, decode=True)
    for i, k in enumerate(names):
        r, s = want(k, flags)
        assert res[i] == r, (k, int(res[i]), r)
        got = out[ooff[i]:ooff[i] + r].tobytes()
        assert got == s, (k, next(j for j in range(r) if got[j] != s[j]))
        assert sizes[i] == len(chunks[i]), (k, int(sizes[i]))
        assert dres[i] == len(chunks[i]) and dout[doff[i]:doff[i] + len(chunks[i])].tobytes() == chunks[i], (k, int(dres[i]))
    assert DB.guards_intact(out, ooff, caps) is None and DB.guards_intact(dout, doff, [len(c) for c in chunks]) is None


@pytest.mark.parametrize("flags", E.FLAGS)
def test_capacities_exact_one_less_and_zero(eng, flags):
    e, N = eng
    names = list(E.cases())
    chunks = [E.cases()[k] for k in names]
    exact = [want(k, flags)[0] for k in names]
    mixed = [x - (i % 2) for i, x in enumerate(exact)]                 # a chunk that fits beside one that does not
    for caps in (exact, [x - 1 for x in exact], [0] * len(names), mixed):
        res, out, ooff = _device_call(e, N, flags, chunks, caps)
        for i, k in enumerate(names):
            if caps[i] >= exact[i]:
                assert res[i] == exact[i] and out[ooff[i]:ooff[i] + exact[i]].tobytes() == want(k, flags)[1], (k, caps[i], int(res[i]))
            else:
                assert res[i] == E.OUT_TOO_SMALL, (k, caps[i], int(res[i]))
        assert DB.guards_intact(out, ooff, caps) is None


PICK = ["text_random_text", "len0", "text4k", "random65537", "len7", "one65537", "huf_fibonacci", "one40", "mlen515"]


def test_batches_of_one_three_and_five_with_mixed_lengths(eng):
    e, N = eng
    for flags in E.FLAGS:
        for part in (PICK[:1], PICK[1:4], PICK[4:9]):
            chunks = [E.cases()[k] for k in part]
            caps = [E.bound(len(c), flags) for c in chunks]
            res, out, ooff = _device_call(e, N, flags, chunks, caps)
            for i, k in enumerate(part):
                assert (int(res[i]), out[ooff[i]:ooff[i] + max(int(res[i]), 0)].tobytes()) == want(k, flags), (k, flags)
            assert DB.guards_intact(out, ooff, caps) is None


def _host_call(e, N, flags, chunks, caps):
    """cj_zstd_compress_batch_host with out_ptrs / out_caps of its own: the inputs at every misalignment, slot i at least G bytes
    behind slot i - 1's end at every misalignment too, the whole output filled with 0xA5 first: (results, output, offsets)"""
    import ctypes as C
    n = len(chunks)
    blob, off, _ = DB.pack(chunks)
    ooff, total = DB.out_slots(caps, mis=DB.out_mis)
    ooff = [int(o) for o in ooff]
    out = np.full(total, 0xA5, np.uint8)
    ins = (C.c_void_p * n)(*[blob.ctypes.data + int(o) for o in off])
    lens = (C.c_size_t * n)(*[len(c) for c in chunks])
    outs = (C.c_void_p * n)(*[out.ctypes.data + o for o in ooff])
    ocaps = (C.c_size_t * n)(*[int(c) for c in caps])
    res = np.zeros(n, np.int64)
    N.check(N.lib().cj_zstd_compress_batch_host(e.h, N.ZSTD_FRAMES, flags, n, ins, lens, outs, ocaps, res.ctypes.data))
    return res, out, ooff


@pytest.mark.parametrize("flags", E.FLAGS)
def test_host_entry_emits_the_models_bytes_at_every_capacity(eng, flags):
    """the C host entry itself, 64 guard bytes around every slot: capacities the bound, exact, exact - 1, 0 and mixed"""
    e, N = eng
    names = list(E.cases())
    chunks = [E.cases()[k] for k in names]
    exact = [want(k, flags)[0] for k in names]
    mixed = [x - (i % 2) for i, x in enumerate(exact)]
    for caps in ([E.bound(len(c), flags) for c in chunks], exact, [x - 1 for x in exact], [0] * len(names), mixed):
        res, out, ooff = _host_call(e, N, flags, chunks, caps)
        for i, k in enumerate(names):
            if caps[i] >= exact[i]:
                assert res[i] == exact[i] and out[ooff[i]:ooff[i] + exact[i]].tobytes() == want(k, flags)[1], (k, caps[i], int(res[i]))
            else:
                assert res[i] == E.OUT_TOO_SMALL, (k, caps[i], int(res[i]))
        assert DB.guards_intact(out, ooff, caps) is None


def test_host_batches_of_one_three_and_five_with_mixed_lengths(eng):
    e, N = eng
    for flags in E.FLAGS:
        for part in (PICK[:1], PICK[1:4], PICK[4:9]):
            chunks = [E.cases()[k] for k in part]
            caps = [E.bound(len(c), flags) for c in chunks]
            res, out, ooff = _host_call(e, N, flags, chunks, caps)
            for i, k in enumerate(part):
                assert (int(res[i]), out[ooff[i]:ooff[i] + max(int(res[i]), 0)].tobytes()) == want(k, flags), (k, flags)
            assert DB.guards_intact(out, ooff, caps) is None


@pytest.mark.parametrize("flags", E.FLAGS)
def test_host_batch_through_python(flags):
    from cramjam_amd import batch
    names = list(E.cases())
    chunks = [E.cases()[k] for k in names]
    cks = bool(flags)
    res, outs = batch.zstd_compress_many(chunks, checksum=cks)
    for k, r, o in zip(names, res, outs):
        assert (r, bytes(o)) == want(k, flags), k
    sub = chunks[:40]
    need = sum(batch.zstd_compress_bound(len(c), cks) for c in sub)
    buf = bytearray(b"\xa5" * (need + 16))
    res2, views = batch.zstd_compress_many(sub, checksum=cks, out=buf)
    assert list(res2) == list(res[:40]) and [bytes(v) for v in views] == [bytes(o) for o in outs[:40]] and bytes(buf[need:]) == b"\xa5" * 16
    back, raw = batch.zstd_decompress_many(outs)
    assert list(back) == [len(c) for c in chunks] and [bytes(x) for x in raw] == [bytes(c) for c in chunks]
    assert list(batch.zstd_sizes(outs)) == [len(c) for c in chunks]
    res3, outs3 = batch.zstd_compress_many(chunks, checksum=cks, devices=[0, 0])          # two host engines on device 0 equal one
    assert list(res3) == list(res) and [bytes(o) for o in outs3] == [bytes(o) for o in outs]
    buf4 = bytearray(b"\xa5" * (need + 16))                                               # the sharded scatter into one buffer through offsets
    res4, views4 = batch.zstd_compress_many(sub, checksum=cks, devices=[0, 0], out=buf4)
    assert [(r, bytes(v)) for r, v in zip(res4, views4)] == [want(k, flags) for k in names[:40]] and bytes(buf4[need:]) == b"\xa5" * 16
    for borrowed in ([bytearray(c) for c in sub], [memoryview(c) for c in sub], [np.frombuffer(c, np.uint8).copy() for c in sub]):
        res5, outs5 = batch.zstd_compress_many(borrowed, checksum=cks)                    # any buffer is borrowed, not copied or converted
        assert [(r, bytes(o)) for r, o in zip(res5, outs5)] == [want(k, flags) for k in names[:40]]
    with pytest.raises((TypeError, ValueError, BufferError)):                             # a buffer that cannot be written is refused, not written
        batch.zstd_compress_many(sub[:2], checksum=cks, out=bytes(need))


def test_twenty_chunks_through_seven_turns_of_a_three_slot_budget(eng):
    e, N = eng
    L = N.lib()
    names = [k for k in E.cases() if len(E.cases()[k]) < 5000][:20]
    assert len(names) == 20
    chunks = [E.cases()[k] for k in names]
    caps = [E.bound(len(c), 1) for c in chunks]
    slot = 262400 + 65536                                             # the records of a piece (16 386 of 16 bytes, to 256), then its literals
    prev = L.cj_debug_zstd_enc_slot_budget(3 * slot)                  # three slots: seven turns
    try:
        res, out, ooff = _device_call(e, N, 1, chunks, caps)
    finally:
        assert L.cj_debug_zstd_enc_slot_budget(prev) == 3 * slot
    for i, k in enumerate(names):
        assert (int(res[i]), out[ooff[i]:ooff[i] + int(res[i])].tobytes()) == want(k, 1), k
    assert DB.guards_intact(out, ooff, caps) is None


def test_five_chunks_of_two_pieces_at_a_budget_below_one_slot(eng):
    """a budget of one byte is one slot: five slices of one chunk each, every frame (with its checksum) what the same call writes at the
    default budget, and read back by the batch decoder"""
    import oracle
    from cramjam_amd import batch
    e, N = eng
    L = N.lib()
    default = 1024 * (262400 + 65536)
    chunks = [oracle.synth_v1(70000, i) for i in range(5)]
    caps = [E.bound(len(c), 1) for c in chunks]
    res0, out0, ooff = _device_call(e, N, 1, chunks, caps)
    assert L.cj_debug_zstd_enc_slot_budget(1) == default              # (the setter returns the previous value)
    try:
        res, out, ooff1 = _device_call(e, N, 1, chunks, caps)
    finally:
        assert L.cj_debug_zstd_enc_slot_budget(0) == 1                # 0: back to the default
    assert L.cj_debug_zstd_enc_slot_budget(0) == default
    assert ooff1 == ooff
    frames = []
    for i in range(5):
        assert int(res[i]) == int(res0[i]) > 0, i
        frames.append(out[ooff[i]:ooff[i] + int(res[i])].tobytes())
        assert frames[i] == out0[ooff[i]:ooff[i] + int(res0[i])].tobytes(), i
    assert [bytes(o) for o in batch.zstd_decompress_many(frames)[1]] == chunks
    assert DB.guards_intact(out, ooff, caps) is None


def test_empty_batches_and_bad_arguments(eng):
    e, N = eng
    L = N.lib()
    from cramjam_amd import batch
    p = e.alloc(64)
    try:
        for flags in E.FLAGS:
            assert L.cj_zstd_compress_batch_device(e.h, N.ZSTD_FRAMES, flags, 0, None, None, None, None, None, None, None, None) == 0
            assert L.cj_zstd_compress_batch_host(e.h, N.ZSTD_FRAMES, flags, 0, None, None, None, None, None) == 0
            assert L.cj_zstd_compress_batch_device(e.h, N.ZSTD_FRAMES, flags, 1, p, p, p, None, p, p, p, None) == E.BAD_ARG
            assert batch.zstd_compress_many([], checksum=bool(flags)) == ([], [])
        for flags in (2, 3, 0x100, 0x80000000):
            assert L.cj_zstd_compress_batch_device(e.h, N.ZSTD_FRAMES, flags, 1, p, p, p, p, p, p, p, None) == E.BAD_ARG
            assert L.cj_zstd_compress_batch_host(e.h, N.ZSTD_FRAMES, flags, 0, None, None, None, None, None) == E.BAD_ARG
        assert L.cj_zstd_compress_batch_device(e.h, 1, 0, 1, p, p, p, p, p, p, p, None) == E.BAD_ARG
        assert L.cj_zstd_compress_batch_host(e.h, 1, 0, 0, None, None, None, None, None) == E.BAD_ARG
        assert L.cj_zstd_batch_device(e.h, N.ZSTD_FRAMES, N.OP_COMPRESS, 0, 1, p, p, p, p, p, p, p, None) == E.BAD_ARG      # still refused there
    finally:
        e.free(p)
    # a limit that belongs to a chunk lands in that chunk's result: an announced length above 0x7E000000 beside a good chunk
    t = E.cases()["text4k"]
    res, out, ooff = _device_call(e, N, 0, [t, t, t], [E.bound(len(t))] * 3, in_lens=[len(t), 0x7E000001, len(t)])
    assert [int(r) for r in res] == [want("text4k", 0)[0], E.INPUT_TOO_LARGE, want("text4k", 0)[0]]
    assert out[ooff[2]:ooff[2] + int(res[2])].tobytes() == want("text4k", 0)[1]


def test_device_entries_on_torch_tensors_on_a_side_stream():
    """zstd_compress_many_device on torch tensors with sync=False, then the decode, in a child that imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(E.ROOT, "tests", "zstd_encode_torch_child.py"), "zstd encode: ok", 600)
