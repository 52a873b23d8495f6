"""ORC compression streams on the GPU (cj_orc_batch_* / cj_orc_sizes_* / cramjam_amd.batch.orc_*), against the model of
tests/orc_model.py and the streams pyarrow's ORC writer wrote (tests/golden/golden_orc.*).  No CPU codec runs here: compressed chunks
are the golden file's, whose decoded bytes are recorded as digests, re-framed by the model, or Python's zlib's.  The device batches go
through the guarded harness of tests/device_batch.py: inputs at every misalignment, 64 guard bytes around every output slot, the
result row filled with UNWRITTEN."""
import ctypes as C
import os

import numpy as np
import pytest

import deflate_cases as D
import device_batch as DB
import orc_model as M

pytestmark = pytest.mark.gpu
CODECS = ("zlib", "snappy", "lz4", "zstd")


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


# ---- chunks and cases ------------------------------------------------------------------------------------------------------------------------
# A chunk: dict(orig, data, size, sha, result) — size: its decoded size as the layout sees it (an original's length, the size query's
# answer, negative: the codec's code); sha: the digest of its decoded bytes; result: the decode's code where it differs from size.
def comp(data, dlen, sha):
    return dict(orig=0, data=data, size=dlen, sha=sha, result=None)


def orig(data):
    return dict(orig=1, data=data, size=len(data), sha=M.digest(data), result=None)


def tiny(codec, k=0):
    """a compressed chunk of about 100 bytes: the stripe footer pyarrow wrote"""
    return comp(*M.golden_chunks(codec, 65536, max_decoded=128)[k])


def bad(codec):
    """a compressed chunk that fails, and where: zlib — block type 3, the size query's CJ_E_DEFLATE_CORRUPT; zstd — a wrong magic, the
    size query's CJ_E_ZSTD_HEADER; lz4 — cut short inside its last literals, the size walk's CJ_E_CORRUPT; snappy — cut short, but the
    size is the header's claim: only the decode finds it, CJ_E_SNAPPY_CORRUPT"""
    t = tiny(codec)
    d = t["data"]
    if codec == "zlib":
        return dict(orig=0, data=bytes([d[0] | 6]) + d[1:], size=-40, sha=None, result=None)
    if codec == "zstd":
        return dict(orig=0, data=b"\x29" + d[1:], size=-50, sha=None, result=None)
    if codec == "lz4":
        return dict(orig=0, data=d[:-3], size=-7, sha=None, result=None)
    return dict(orig=0, data=d[:-3], size=t["size"], sha=None, result=-12)


def case(chunks, bs, cap=None, walk_tail=b"", after=b""):
    """one stream of the chunks (walk_tail: bytes behind the last one that break the walk) with the model's verdict"""
    s = M.frame([(c["orig"], c["data"]) for c in chunks]) + walk_tail
    sizes = [c["size"] for c in chunks]
    room = sum(v for v in sizes if 0 <= v <= bs)
    cap = room if cap is None else cap
    want = M.verdict(M.walk(s)[0], sizes, bs, cap, [c["result"] for c in chunks])
    late = want < 0 and any(c["result"] is not None for c in chunks) and M.verdict(M.walk(s)[0], sizes, bs, cap) >= 0
    return dict(bytes=s, cap=cap, result=want, sizes=sizes, parts=[(c["size"], c["sha"]) for c in chunks] if want >= 0 else [], after=after,
                written=cap if late else 0)      # only a stream whose chunk fails in the decode may have written, inside its slot


def run_device(e, N, codec, bs, cases, sizes=False, after=True):
    """one guarded device batch over the cases, held to the model's results, to the recorded digests chunk by chunk, and to the mask:
    nothing outside [0, result) of an accepted stream, nothing at all for a stream refused before the decode.  Returns the results."""
    n, L, kind = len(cases), N.lib(), M.KINDS[codec]
    blob, off, lens = DB.pack([c["bytes"] for c in cases], [c["after"] if after else b"" for c in cases])
    caps = np.array([c["cap"] for c in cases], np.uint64)
    want = np.array([c["result"] for c in cases], np.int64)
    ooff, total = DB.out_slots(caps, mis=DB.out_mis)
    if sizes:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_orc_sizes_device(e.h, kind, 0, bs, n, i, o, l, r, None))
    else:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_orc_batch_device(e.h, kind, N.OP_DECOMPRESS, 0, bs, n, i, o, l, out, oo, oc, r, None))
    res, out, blob_after = DB.run(e, call, blob, off, lens, ooff, caps, total, with_input=True, what=("orc", codec, bs))
    tag = lambda i: (codec, bs, i, int(res[i]), int(want[i]))
    DB.check_results(res, want, tag)
    keep = DB.untouched(ooff, want, total, written=[c["written"] for c in cases], sized=sizes)
    DB.check_mask(out, keep, ooff, tag)
    assert DB.guards_intact(out, ooff, caps) is None and (blob_after == blob).all()
    if not sizes:
        for i, c in enumerate(cases):
            p = int(ooff[i])
            for dlen, sha in c["parts"]:
                assert M.digest(out[p:p + dlen]) == sha, ("bytes", tag(i))
                p += dlen
    return [int(r) for r in res]


def edge_cases(codec, bs=4096):
    """the wave-round edges of the layout and verdict kernels, and the header edges, as one batch"""
    t, b = tiny(codec), bad(codec)
    neighbour = M.frame([(0, t["data"]), (1, b"behind the end")])             # what a read past the input's end would take for a chunk
    mix = lambda n: [orig(b"original chunk %03d of this stream......" % k) if k % 5 == 4 else t for k in range(n)]
    big = orig(bytes(bs + 1))                                                   # more than a block: CJ_E_ORC_BLOCK
    cases = [case(mix(n), bs, after=neighbour) for n in (0, 1, 63, 64, 65, 130)]
    for at3, at70 in ((b, big), (big, b), (None, b), (b, None), (b, b), (None, big)):
        ch = mix(130)
        if at3 is not None:
            ch[3] = at3
        if at70 is not None:
            ch[70] = at70
        cases.append(case(ch, bs, after=neighbour))
    # header edges
    cases += [case([], bs, walk_tail=b"\x01", after=b"\x00\x00" + neighbour), case([], bs, walk_tail=b"\x01\x00", after=b"\x00" + neighbour),
              case([t], bs, walk_tail=M.header(6, 1) + b"12345", after=b"6" + neighbour),      # a chunk whose length passes the end by 1
              case([orig(b"")] * 3000, bs, after=neighbour), case([orig(b""), t, orig(b"")], bs), case([t, t], bs, cap=2 * t["size"] - 1),
              case([t, orig(b"xyz")], bs, cap=t["size"] + 3), case([t, orig(b"xyz")], bs, cap=t["size"] + 2, after=neighbour)]
    return cases


# ---- decode --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
def test_golden_streams_host_and_device(eng, codec):
    from cramjam_amd import batch
    e, N = eng
    for bs in (65536, 262144):
        gs = M.golden_of(codec, bs)
        streams, lens = [g["stream"] for g in gs], [g["decoded_len"] for g in gs]
        assert batch.orc_stream_sizes(streams, codec, bs) == lens
        for res, outs in (batch.orc_decompress_streams(streams, codec, bs), batch.orc_decompress_streams(streams, codec, bs, output_lens=lens)):
            assert list(res) == lens and [M.digest(o) for o in outs] == [g["sha256"] for g in gs], (codec, bs)
        cases = [dict(bytes=g["stream"], cap=g["decoded_len"], result=g["decoded_len"], parts=[(c[3], c[4]) for c in g["chunks"]], after=b"", written=0) for g in gs]
        run_device(e, N, codec, bs, cases)
        run_device(e, N, codec, bs, cases, sizes=True)
    assert batch.orc_stream_sizes([], codec) == [] and batch.orc_decompress_streams([], codec) == ([], [])


def test_the_edge_cases_cover_what_they_promise():
    for codec in CODECS:
        cs = edge_cases(codec)
        want = [c["result"] for c in cs]
        assert want[0] == 0 and want[1] == 100 and all(w > 0 for w in want[1:6])
        assert want[6] == bad(codec)["size"] if codec != "snappy" else want[6] == M.ORC_BLOCK      # (3, 70): the earlier position — Snappy's only fails in the decode, behind the layout
        assert want[7] == M.ORC_BLOCK and want[11] == M.ORC_BLOCK
        assert want[8] == want[9] == want[10] == (bad(codec)["size"] if codec != "snappy" else -12)
        assert want[12:15] == [M.ORC_HEADER] * 3 and want[15] == 0 and want[16] == 100 and want[17] == M.OUT_TOO_SMALL
        assert want[18] == 103 and want[19] == M.OUT_TOO_SMALL


@pytest.mark.parametrize("codec", CODECS)
def test_wave_round_and_header_edges_and_capacities(eng, codec):
    e, N = eng
    cases = edge_cases(codec)
    got = run_device(e, N, codec, 4096, cases)
    assert run_device(e, N, codec, 4096, cases, after=False) == got                     # whatever lies behind an input: the same results
    run_device(e, N, codec, 4096, [sized(c, 4096) for c in cases], sizes=True)


def sized(c, bs):
    """the case as the size query answers it: no capacity, no decode"""
    return dict(c, result=M.verdict(M.walk(c["bytes"])[0], c["sizes"], bs))


@pytest.mark.parametrize("codec", CODECS)
def test_block_edges(eng, codec):
    e, N = eng
    full = comp(*M.golden_chunks(codec, 65536, min_decoded=65536)[0])
    cases = [case([full], 65536), case([orig(bytes(65536))], 65536), case([orig(bytes(65537))], 65536), case([full, orig(b""), full], 65536)]
    assert [c["result"] for c in cases] == [65536, 65536, M.ORC_BLOCK, 131072]
    run_device(e, N, codec, 65536, cases)
    over = [case([full], 65535), case([orig(bytes(65535))], 65535), case([tiny(codec), full], 65535)]
    assert [c["result"] for c in over] == [M.ORC_BLOCK, 65535, M.ORC_BLOCK]
    run_device(e, N, codec, 65535, over)


def test_block_edges_at_4096_with_zlib(eng):
    e, N = eng
    text = D.words(4097, 61)
    z = lambda b: comp(M.deflate_raw(b), len(b), M.digest(b))
    cases = [case([z(text[:4096])], 4096), case([z(text)], 4096), case([orig(text[:4096])], 4096), case([orig(text)], 4096), case([orig(b"")], 4096),
             case([z(text[:4096]), orig(b""), z(text[:4095])], 4096)]
    assert [c["result"] for c in cases] == [4096, M.ORC_BLOCK, 4096, M.ORC_BLOCK, 0, 8191]
    run_device(e, N, "zlib", 4096, cases)
    run_device(e, N, "zlib", 4096, [sized(c, 4096) for c in cases], sizes=True)


@pytest.mark.parametrize("codec", ("lz4", "snappy"))
def test_big_chunks(eng, codec):
    """one 262 144-byte compressed chunk: the engine's big-chunk path"""
    e, N = eng
    full = comp(*M.golden_chunks(codec, 262144, min_decoded=262144)[0])
    cases = [case([full], 262144), case([tiny(codec), full, orig(b"tail")], 262144)]
    assert [c["result"] for c in cases] == [262144, 262144 + 104]
    run_device(e, N, codec, 262144, cases)


def test_dirty_scratch(eng):
    """the same batch after batches of other codecs and sizes have used the engine's scratch, and after every scratch buffer was filled"""
    e, N = eng
    L = N.lib()
    cases = edge_cases("zlib")
    first = run_device(e, N, "zlib", 4096, cases)
    gs = M.golden_of("lz4", 65536)
    big = [dict(bytes=g["stream"], cap=g["decoded_len"], result=g["decoded_len"], parts=[(c[3], c[4]) for c in g["chunks"]], after=b"", written=0) for g in gs]
    run_device(e, N, "lz4", 65536, big)
    assert run_device(e, N, "zlib", 4096, cases) == first
    filled = (C.c_uint64 * L.cj_debug_scratch_count())()
    for pattern in (1, 2 + 0x5EED):
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        assert run_device(e, N, "zlib", 4096, cases) == first
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        run_device(e, N, "lz4", 65536, big)


# ---- encode --------------------------------------------------------------------------------------------------------------------------------
def enc_buffers(bs):
    rnd = np.random.default_rng(11).integers(0, 256, 3 * bs + 5, dtype=np.uint8).tobytes()
    text = D.words(3 * bs + 5, 79)
    sizes = (0, 1, bs - 1, bs, bs + 1, 3 * bs + 5)
    return [text[:n] for n in sizes] + [rnd[:n] for n in sizes], len(sizes)


def slot_stride(L, N, codec, bs):
    b = {"zlib": lambda: L.cj_deflate_compress_bound(bs, N.DEFLATE_RAW), "snappy": lambda: L.cj_snappy_raw_max_compress_len(bs),
         "lz4": lambda: L.cj_lz4_block_compress_bound(bs, 0), "zstd": lambda: L.cj_zstd_compress_bound(bs, 0)}[codec]()
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("bs", (4096, 65536))
@pytest.mark.parametrize("codec", CODECS)
def test_encode(eng, codec, bs):
    from cramjam_amd import batch
    e, N = eng
    L = N.lib()
    bufs, half = enc_buffers(bs)
    res, outs = batch.orc_compress_streams(bufs, codec, bs)
    outs = [bytes(o) for o in outs]
    for i, (b, r, s) in enumerate(zip(bufs, res, outs)):
        assert r == len(s), (i, r)
        chunks = M.check_encoded(s, b, bs, codec, random_input=i >= half and len(b) >= 64)
        if i < half and len(b) >= bs - 1:
            assert not any(o for _, _, o in chunks[:len(b) // bs]), ("a full piece of text stayed original", i)
    assert outs[0] == b"" and outs[1] == M.frame([(1, bufs[1])])                      # an empty buffer is an empty stream; one byte stays original
    back, raw = batch.orc_decompress_streams(outs, codec, bs)
    assert list(back) == [len(b) for b in bufs] and [bytes(x) for x in raw] == bufs
    assert batch.orc_stream_sizes(outs, codec, bs) == [len(b) for b in bufs]
    # two shards, both on engine 0, give the single-engine result
    res2, outs2 = batch.orc_compress_streams(bufs, codec, bs, devices=[0, 0])
    assert list(res2) == list(res) and [bytes(o) for o in outs2] == outs
    back2, raw2 = batch.orc_decompress_streams(outs, codec, bs, devices=[0, 0])
    assert list(back2) == list(back) and [bytes(x) for x in raw2] == bufs
    # the device entry in the harness: the bound suffices, one byte less is refused with nothing written
    bound = [batch.orc_compress_bound(len(b), bs) for b in bufs]
    kind, n = M.KINDS[codec], len(bufs)
    call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_orc_batch_device(e.h, kind, N.OP_COMPRESS, 0, bs, n, i, o, l, out, oo, oc, r, None))
    for caps in (bound, [max(c - (i % 2), 0) for i, c in enumerate(bound)]):
        got, out, ooff = DB.run_chunks(e, call, bufs, caps, out_mis=DB.out_mis)
        for i, s in enumerate(outs):
            if caps[i] >= bound[i]:
                assert got[i] == len(s) and out[ooff[i]:ooff[i] + len(s)].tobytes() == s, (i, int(got[i]))
                assert (out[ooff[i] + len(s):ooff[i] + caps[i]] == DB.FILL).all(), i
            else:
                assert got[i] == M.OUT_TOO_SMALL and (out[ooff[i]:ooff[i] + caps[i]] == DB.FILL).all(), (i, int(got[i]))
        assert DB.guards_intact(out, ooff, caps) is None
    # three turns of the chunk slots give the same bytes
    npieces = sum(-(-len(b) // bs) for b in bufs)
    per = -(-npieces // 3)
    assert -(-npieces // per) == 3
    budget = per * slot_stride(L, N, codec, bs)
    prev = L.cj_debug_orc_slot_budget(budget)
    try:
        res3, outs3 = batch.orc_compress_streams(bufs, codec, bs)
    finally:
        assert L.cj_debug_orc_slot_budget(prev) == budget
    assert list(res3) == list(res) and [bytes(o) for o in outs3] == outs
    # the `out=` form equals the `bytes` form
    buf = bytearray(b"\xa5" * (sum(bound) + 16))
    res4, views = batch.orc_compress_streams(bufs, codec, bs, out=buf)
    assert list(res4) == list(res) and [bytes(v) for v in views] == outs and bytes(buf[sum(bound):]) == b"\xa5" * 16


@pytest.mark.parametrize("codec", CODECS)
def test_streams_across_turns_through_the_device_entry(eng, codec):
    """Two chunk slots a turn, and streams without a piece — empty ones, refused ones — at and next to the turn edges: pieces 0 | 1 2 3 |
    4 5 6 7 | 8 9 of streams 1, 4, 6 and 8 go through the turns (0 1)(2 3)(4 5)(6 7)(8 9), so the piece-less streams 2, 3 share piece 1
    with stream 4, stream 5 shares piece 4 — a turn's first — with stream 6, and stream 7 piece 8 with stream 8.  The bytes are those
    of the host call with the default budget, one turn."""
    from cramjam_amd import batch
    e, N = eng
    L, bs = N.lib(), 4096
    text = D.words(3 * bs, 83)
    rnd = np.random.default_rng(12).integers(0, 256, 3 * bs + 5, dtype=np.uint8).tobytes()
    bufs = [b"", b"x", text[:2 * bs + 100], b"", text[100:3 * bs], text[:100], rnd, b"", text[7:bs + 8]]
    refused = (2, 5)
    assert [-(-len(b) // bs) for b in bufs] == [0, 1, 3, 0, 3, 1, 4, 0, 2]
    res, outs = batch.orc_compress_streams(bufs, codec, bs)
    outs = [bytes(o) for o in outs]
    for i, (b, r, s) in enumerate(zip(bufs, res, outs)):
        assert r == len(s), (i, r)
        M.check_encoded(s, b, bs, codec, random_input=i == 6)
    bound = [batch.orc_compress_bound(len(b), bs) for b in bufs]
    caps = [c - 1 if i in refused else c for i, c in enumerate(bound)]
    kind, n = M.KINDS[codec], len(bufs)
    call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_orc_batch_device(e.h, kind, N.OP_COMPRESS, 0, bs, n, i, o, l, out, oo, oc, r, None))
    budget = 2 * slot_stride(L, N, codec, bs)
    prev = L.cj_debug_orc_slot_budget(budget)
    try:
        got, out, ooff = DB.run_chunks(e, call, bufs, caps, out_mis=DB.out_mis)
    finally:
        assert L.cj_debug_orc_slot_budget(prev) == budget
    for i, s in enumerate(outs):
        if i in refused:
            assert got[i] == M.OUT_TOO_SMALL and (out[ooff[i]:ooff[i] + caps[i]] == DB.FILL).all(), (i, int(got[i]))
        else:
            assert got[i] == len(s) and out[ooff[i]:ooff[i] + len(s)].tobytes() == s, (i, int(got[i]))
            assert (out[ooff[i] + len(s):ooff[i] + caps[i]] == DB.FILL).all(), i
    assert DB.guards_intact(out, ooff, caps) is None


def test_device_entries_on_torch_tensors():
    """orc_compress_streams_device, orc_stream_sizes_device and orc_decompress_streams_device on torch tensors on a side stream, in a
    child that imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(D.ROOT, "tests", "orc_torch_child.py"), "orc torch: ok", 600)
