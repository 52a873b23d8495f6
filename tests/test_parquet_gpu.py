"""Parquet column chunks on the GPU (cj_parquet_batch_* / cj_parquet_sizes_* / cj_parquet_pages_* / cramjam_amd.batch.parquet_*;
DESIGN.md 5.18), against the model of tests/parquet_model.py and the chunks pyarrow's writer wrote (tests/golden/golden_parquet*).  No
CPU codec runs here: page bodies are the golden files', whose decoded bytes lie in the uncompressed file, re-framed by the model's
header writer.  Where a rule says "the decoder's code", the decoder's plain batch gives it, for the same body at the same capacity.
The device batches go through the guarded harness of tests/device_batch.py: inputs at every misalignment, 64 guard bytes around every
output slot, the result row filled with UNWRITTEN."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import device_batch as DB
import parquet_model as M

pytestmark = pytest.mark.gpu
ALL = tuple(M.CODECS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


# ---- pages and cases -----------------------------------------------------------------------------------------------------------------------
_plain = {}


def plain_result(codec, body, cap):
    """what the codec's plain batch gives for `body` at capacity `cap`: (result, bytes) — the reference for "the decoder's code" """
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    key = (codec, bytes(body), cap)
    if key not in _plain:
        what, kind = {"snappy": (N.CODEC_SNAPPY_RAW, N.BLOCKS), "lz4_raw": (N.CODEC_LZ4_BLOCK, N.BLOCKS), "gzip": (N.DEFLATE_GZIP, N.DEFLATE), "zstd": (N.ZSTD_FRAMES, N.ZSTD)}[codec]
        res, outs = batch._run(what, N.OP_DECOMPRESS, 0, [bytes(body)], [cap], None, kind=kind)
        _plain[key] = int(res[0]), bytes(outs[0])
    return _plain[key]


def small(codec, k=0):
    """the k-th small page body of a codec as (bytes in the file, decoded bytes); "uncompressed": the decoded bytes themselves"""
    src = M.bodies("zstd" if codec == "uncompressed" else codec, max_decoded=600)
    body, dec = src[k % len(src)]
    return (dec, dec) if codec == "uncompressed" else (body, dec)


def pg(codec, k=0, state=0, **kw):
    """one V1 page of small(codec, k) that states `state` bytes more than it decodes to: (page bytes, the codec's result or None, the
    bytes it leaves in its room — FILL where nothing is written)"""
    body, dec = small(codec, k)
    usize = len(dec) + state
    if codec == "uncompressed":
        r, left = None, dec[:usize] + bytes([DB.FILL]) * max(state, 0)
    else:
        r = plain_result(codec, body, usize)[0]
        left = (dec + bytes([DB.FILL]) * usize)[:usize] if r >= 0 else None      # (a result that is not len(dec) fails the chunk: then nothing is compared)
        r = None if r == usize else r
    return M.page(body, usize, **kw), r, left


def case(codec, pages, cap=None, verify=False, after=b"", tail=b""):
    """one chunk of pg()-style pages (tail: bytes behind the last page that break the walk) with the model's verdict"""
    chunk = b"".join(p[0] for p in pages) + tail
    results = [p[1] for p in pages]
    room = M.verdict(chunk, codec)
    cap = max(room, 0) if cap is None else cap
    want = M.verdict(chunk, codec, cap, results, verify)
    late = want < 0 and M.verdict(chunk, codec, cap) >= 0                       # a page failed in the decode (a decoder's -6 too): the chunk may have written inside its slot
    out = b"".join(p[2] for p in pages) if want >= 0 and all(p[2] is not None for p in pages) else None
    return dict(bytes=chunk, cap=cap, result=want, out=out, after=after, written=cap if late else 0)


def run_device(e, N, codec, cases, verify=False, sizes=False, after=True):
    """one guarded device batch over the cases, held to the model's results, to the expected bytes, and to the mask: nothing outside
    [0, result) of an accepted chunk, nothing at all for a chunk refused before the decode.  Returns the results."""
    n, L, what = len(cases), N.lib(), M.CODECS[codec]
    blob, off, lens = DB.pack([c["bytes"] for c in cases], [c["after"] if after else b"" for c in cases])
    caps = np.array([c["cap"] for c in cases], np.uint64)
    want = np.array([c["result"] for c in cases], np.int64)
    ooff, total = DB.out_slots(caps, mis=DB.out_mis)
    if sizes:
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_parquet_sizes_device(e.h, what, 0, n, i, o, l, r, None))
    else:
        flags = N.PARQUET_FLAG_VERIFY_CRC if verify else 0
        call = lambda i, o, l, out, oo, oc, r: N.check(L.cj_parquet_batch_device(e.h, what, N.OP_DECOMPRESS, flags, n, i, o, l, out, oo, oc, r, None))
    res, out, blob_after = DB.run(e, call, blob, off, lens, ooff, caps, total, with_input=True, what=("parquet", codec, verify, sizes))
    tag = lambda i: (codec, verify, i, int(res[i]), int(want[i]))
    DB.check_results(res, want, tag)
    keep = DB.untouched(ooff, want, total, written=[c["written"] for c in cases], sized=sizes)
    DB.check_mask(out, keep, ooff, tag)
    assert DB.guards_intact(out, ooff, caps) is None and (blob_after == blob).all()
    if not sizes:
        for i, c in enumerate(cases):
            if c["out"] is not None:
                got = out[int(ooff[i]):int(ooff[i]) + (len(c["out"]) if isinstance(c["out"], bytes) else c["out"][0])].tobytes()
                assert (got == c["out"]) if isinstance(c["out"], bytes) else (M.digest(got) == c["out"][1]), ("bytes", tag(i))
    return [int(r) for r in res]


def sized(c, codec):
    return dict(c, result=M.verdict(c["bytes"], codec), out=None)


def golden_cases(codec, big=None):
    return [dict(bytes=g["chunk"], cap=g["decoded_len"], result=g["decoded_len"], out=(g["decoded_len"], g["sha256"]), after=b"", written=0, g=g) for g in M.golden_of(codec, big=big)]


# ---- the golden chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ALL)
def test_golden_chunks_host_and_device(eng, codec):
    """every golden chunk as a host batch and a device batch: results, digests, sizes and page tables, with and without the CRCs"""
    from cramjam_amd import batch
    e, N = eng
    cases = golden_cases(codec)
    gs = [c["g"] for c in cases]
    chunks, lens = [g["chunk"] for g in gs], [g["decoded_len"] for g in gs]
    assert len(gs) == 15 and batch.parquet_chunk_sizes(chunks, codec) == lens
    runs = (batch.parquet_decompress_chunks(chunks, codec), batch.parquet_decompress_chunks(chunks, codec, output_lens=lens, verify_crc=True),
            batch.parquet_decompress_chunks(chunks, codec, output_lens=[g["total_uncompressed_size"] for g in gs], devices=[0, 0]))      # the footer's size suffices
    for res, outs in runs:
        assert list(res) == lens and [M.digest(o) for o in outs] == [g["sha256"] for g in gs], codec
    tabs = batch.parquet_pages(chunks)
    assert [t.tolist() for t in tabs] == [g["pages"] for g in gs]
    got = run_device(e, N, codec, cases)
    assert run_device(e, N, codec, cases, verify=True) == got == lens
    run_device(e, N, codec, [sized(c, codec) for c in cases], sizes=True)
    assert batch.parquet_chunk_sizes([], codec) == [] and batch.parquet_decompress_chunks([], codec) == ([], []) and batch.parquet_pages([]) == []


@pytest.mark.parametrize("codec", M.REAL)
def test_large_page(eng, codec):
    """one page of at least 100 000 bytes: beyond the workgroup decoder's 64 KiB for Snappy and LZ4"""
    e, N = eng
    cases = golden_cases(codec, big=True)
    assert len(cases) == 1 and cases[0]["g"]["pages"][0][3] >= 100000
    one = cases[0]
    two = dict(one, bytes=pg(codec)[0] + one["bytes"], cap=one["cap"] + len(small(codec)[1]), out=None)
    two["result"] = two["cap"]
    run_device(e, N, codec, [one, two], verify=True)
    run_device(e, N, codec, [dict(one, cap=one["cap"] - 1, result=M.OUT_TOO_SMALL, out=None)])


# ---- page counts, page order ---------------------------------------------------------------------------------------------------------------
def count_cases(codec, verify=False):
    neighbour = pg(codec, 1)[0]                                                 # what a read past the input's end would take for a page
    mix = lambda n: [pg(codec, k) if k % 5 else pg(codec, k, crc=None) for k in range(n)]
    cases = [case(codec, mix(n), verify=verify, after=neighbour) for n in (0, 1, 63, 64, 65, 130)]
    more, less = pg(codec, 3, +1), pg(codec, 3, -1)                             # SIZE, the decoder's code (no codec: neither is checked)
    for at3, at70 in ((more, less), (less, more), (None, less), (more, None)):
        ps = mix(130)
        for at, p in ((3, at3), (70, at70)):
            if p is not None:
                ps[at] = p
        cases.append(case(codec, ps, verify=verify, after=neighbour))
    return cases


@pytest.mark.parametrize("codec", ALL)
def test_page_counts_and_page_order(eng, codec):
    e, N = eng
    cases = count_cases(codec)
    want = [c["result"] for c in cases]
    assert want[0] == 0 and all(w > 0 for w in want[1:6])
    if codec != "uncompressed":
        more, less = pg(codec, 3, +1), pg(codec, 3, -1)
        assert more[1] is not None and more[1] >= 0 and less[1] is not None and less[1] < 0, "one byte more ends well and short; one byte less is the decoder's to refuse"
        assert want[6:] == [M.SIZE, less[1], less[1], M.SIZE]                   # the first page in page order, whichever code it has
    got = run_device(e, N, codec, cases)
    assert run_device(e, N, codec, cases, after=False) == got                   # whatever lies behind an input: the same results
    assert run_device(e, N, codec, count_cases(codec, True), verify=True) == got
    run_device(e, N, codec, [sized(c, codec) for c in cases], sizes=True)


# ---- the CRC -------------------------------------------------------------------------------------------------------------------------------
def flipped_cases(codec, verify):
    """a 65-page chunk with one payload bit flipped in page 0 / in page 64; then, in a V2 page's levels, which no decoder sees"""
    cases = []
    for at in (0, 64):
        ps = [pg(codec, k) for k in range(65)]
        body, dec = small(codec, at)
        bad = bytearray(body)
        bad[len(bad) // 2] ^= 0x10
        if codec == "uncompressed":
            r, left = None, bytes(bad)
        else:
            r, got = plain_result(codec, bytes(bad), len(dec))
            r, left = (None if r == len(dec) else r), None
        ps[at] = (M.header(0, len(dec), len(body), zlib.crc32(body)) + bytes(bad), r, left)
        cases.append(case(codec, ps, verify=verify))
        assert not verify or cases[-1]["result"] == M.CRC
    body, dec = small(codec)
    lv = b"\x03\x00\x00\x00levels!"
    v2 = M.header(M.DATA_PAGE_V2, len(dec) + len(lv), len(body) + len(lv), zlib.crc32(lv + body), def_len=4, rep_len=len(lv) - 4) + b"\x07" + lv[1:] + body
    cases.append(case(codec, [pg(codec, 1), (v2, None, b"\x07" + lv[1:] + dec), pg(codec, 2)], verify=verify))
    assert cases[-1]["result"] == (M.CRC if verify else len(dec) + len(lv) + len(small(codec, 1)[1]) + len(small(codec, 2)[1]))
    return cases


@pytest.mark.parametrize("codec", ALL)
def test_flipped_bits_are_the_crcs_to_find(eng, codec):
    e, N = eng
    assert run_device(e, N, codec, flipped_cases(codec, True), verify=True) == [M.CRC] * 3
    run_device(e, N, codec, flipped_cases(codec, False))                        # without the flag: the decoder's own result


# ---- size and CRC rules, capacities, header ends ---------------------------------------------------------------------------------------------
def rule_cases(codec, verify):
    a, b, c = pg(codec, 0), pg(codec, 1), pg(codec, 2)
    body, dec = small(codec)
    flat = (M.page(dec, len(dec) + 1, type=M.DATA_PAGE_V2, is_compressed=False), None, dec + bytes([DB.FILL]))      # copied, not held to its size
    shorter = (M.page(dec, len(dec) - 1, type=M.DATA_PAGE_V2, is_compressed=False), None, dec[:-1])                 # ... and never beyond its room
    lv = b"\x02\x00\x00\x00ab"
    levels = (M.page(lv + body, len(lv) + len(dec), type=M.DATA_PAGE_V2, def_len=6, is_compressed=None if codec != "uncompressed" else False), None, lv + dec)
    empty = (M.page(lv, len(lv), type=M.DATA_PAGE_V2, rep_len=2, def_len=4), None, lv)                              # 0 bytes of values that state 0 bytes
    skip = (M.page(b"an index page, not read", 23, type=M.INDEX_PAGE, crc=12345), None, b"")                        # its CRC is not looked at
    nobytes = (M.page(b"", 0, crc=0), None, b"")
    badsum = (M.page(b"", 0, crc=5), None, b"")
    stated = sum(len(p[2]) for p in (a, b, c))
    neighbour = a[0]
    cases = [case(codec, [a, pg(codec, 1, +1), c], verify=verify), case(codec, [a, pg(codec, 1, -1), c], verify=verify),
             case(codec, [a, flat, b], verify=verify), case(codec, [a, shorter, b], verify=verify), case(codec, [levels, a, empty, b], verify=verify),
             case(codec, [a, skip, b, skip], verify=verify), case(codec, [a, nobytes, b], verify=verify), case(codec, [a, badsum, b], verify=verify),
             case(codec, [a, b, c], verify=verify), case(codec, [a, b, c], cap=stated - 1, verify=verify, after=neighbour), case(codec, [a, b, c], cap=stated + 7, verify=verify),
             case(codec, [a, b], tail=c[0][:5], verify=verify, after=c[0][5:]),                       # ends inside a header
             case(codec, [a, b], tail=c[0][:-1], verify=verify, after=c[0][-1:] + neighbour),         # one byte short of its payload
             case(codec, [], tail=b"\x15", verify=verify, after=a[0][1:])]
    return cases


@pytest.mark.parametrize("codec", ALL)
def test_size_and_crc_rules_and_capacities(eng, codec):
    e, N = eng
    cases = rule_cases(codec, False)
    want = [c["result"] for c in cases]
    stated, (la, lb) = cases[8]["result"], (len(small(codec, k)[1]) for k in (0, 1))
    if codec != "uncompressed":
        assert want[0] == M.SIZE and want[1] == pg(codec, 1, -1)[1] < 0
    assert want[2] == 2 * la + lb + 1 and want[3] == 2 * la + lb - 1 and want[4] == 2 * la + lb + 12 and want[5] == want[6] == want[7] == want[8] - len(small(codec, 2)[1])
    assert want[8:] == [stated, M.OUT_TOO_SMALL, stated, M.HEADER, M.HEADER, M.HEADER] and [c["written"] for c in cases[9:]] == [0, 0, 0, 0, 0]
    got = run_device(e, N, codec, cases)
    assert run_device(e, N, codec, cases, after=False) == got
    checked = rule_cases(codec, True)
    assert [c["result"] for c in checked][7] == M.CRC and [c["result"] for k, c in enumerate(checked) if k != 7] == [w for k, w in enumerate(want) if k != 7]
    run_device(e, N, codec, checked, verify=True)
    run_device(e, N, codec, [sized(c, codec) for c in cases], sizes=True)


# ---- the pages query -------------------------------------------------------------------------------------------------------------------------
def test_pages_query_on_the_device(eng):
    """rows null: the counts; an exact row_cap: the tables; one row too few: refused, nothing written; a chunk the walk refuses: its code"""
    e, N = eng
    L = N.lib()
    gs = M.golden_of("snappy", 2, big=False) + M.golden_of("gzip", 1)
    chunks = [g["chunk"] for g in gs] + [b"", pg("zstd")[0][:-1], M.page(b"index", 5, type=M.INDEX_PAGE, crc=None) + pg("zstd")[0]]
    tables = [g["pages"] for g in gs] + [[], None, M.table(M.walk(chunks[-1])[1])]
    n = len(chunks)
    counts = [len(t) if t is not None else M.HEADER for t in tables]
    assert counts[-1] == 2 and tables[-1][1][4] == 0                            # a skipped page takes no room in the output
    blob, off, lens = DB.pack(chunks, [pg("zstd", 1)[0]] * n)
    for short in (None, 0, 1):
        caps = np.array([max(c, 0) - (1 if short is not None and k % 2 == short and c > 0 else 0) for k, c in enumerate(counts)], np.uint64)
        want = np.array([M.OUT_TOO_SMALL if c > cap else c for c, cap in zip(counts, caps)], np.int64)
        ooff, total = DB.out_slots(caps * 64)
        assert not (ooff % 64).any()
        with DB.device_batch(e, blob, off, lens, ooff, caps * 64, total, what="parquet pages") as b:
            d_in, p_off, p_len, d_out, _, _, p_res = b.args
            row_off, row_cap = b.rows(ooff // 64, caps)
            N.check(L.cj_parquet_pages_device(e.h, 0, n, d_in, p_off, p_len, None, None, None, p_res, None))
            e.sync()
            assert b.read_row(p_res).tolist() == counts
            e.h2d(p_res, np.full(n, DB.UNWRITTEN, np.uint64))
            N.check(L.cj_parquet_pages_device(e.h, 0, n, d_in, p_off, p_len, d_out, row_off, row_cap, p_res, None))
            res, out = b.read()
        tag = lambda i: ("pages", short, i, int(res[i]), int(want[i]))
        DB.check_results(res, want, tag)
        DB.check_mask(out, DB.untouched(ooff, np.maximum(want, 0) * 64, total), ooff, tag)
        for i, t in enumerate(tables):
            if want[i] > 0:
                assert out[int(ooff[i]):int(ooff[i]) + 64 * len(t)].view(np.int64).reshape(-1, 8).tolist() == t, tag(i)
    from cramjam_amd import batch
    tabs = batch.parquet_pages(chunks, devices=[0, 0])
    assert [t if isinstance(t, int) else t.tolist() for t in tabs] == [t if t is not None else M.HEADER for t in tables]


# ---- the engine's other invariants -----------------------------------------------------------------------------------------------------------
def test_dirty_scratch(eng):
    """the same batch after batches of other codecs and sizes have used the engine's scratch, and after every scratch buffer was filled"""
    e, N = eng
    L = N.lib()
    cases = count_cases("gzip", True) + rule_cases("gzip", True)
    first = run_device(e, N, "gzip", cases, verify=True)
    big = golden_cases("lz4_raw")
    run_device(e, N, "lz4_raw", big)
    run_device(e, N, "zstd", golden_cases("zstd", big=False), verify=True)
    assert run_device(e, N, "gzip", cases, verify=True) == first
    filled = (C.c_uint64 * L.cj_debug_scratch_count())()
    for pattern in (1, 2 + 0x5EED):
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        assert run_device(e, N, "gzip", cases, verify=True) == first
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        run_device(e, N, "lz4_raw", big, verify=True)
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        run_device(e, N, "snappy", count_cases("snappy"))


def test_device_entries_on_torch_tensors():
    """parquet_decompress_chunks_device, parquet_chunk_sizes_device and parquet_pages_device on torch tensors on a side stream, the two
    queries with sync=False, in a child that imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(ROOT, "tests", "parquet_torch_child.py"), "parquet torch: ok", 600)
