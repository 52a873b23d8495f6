"""The Parquet writer without a GPU: the model's rules (tests/parquet_write_model.py) read back by the reader's model;
the host build of the header writer (cramjam_amd/csrc/parquet_write.hpp, unchanged, tests/hostsim/sim_parquet_write.cpp) against
parquet_model.header() byte for byte — the fields of every golden page, every varint length edge, the CRCs that are negative I32s, the
three page types, both flag values —, its length, parquet_grammar.hpp's reader over every written header, the maximal header; the same
as a stand-alone program under AddressSanitizer and UBSan with every destination flush against the end of its allocation; the slot
bound against the encoders' bounds; cj_parquet_compress_bound against the model's worst case; the argument checks that need no device."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import pytest

import parquet_model as M
import parquet_write_model as W
from hostsim_build import SANITIZE, build_sim

WORDS = ("type", "usize", "csize", "crc", "has_crc", "num_values", "num_nulls", "num_rows", "encoding", "def_enc", "rep_enc", "def_len", "rep_len", "is_compressed")
I32_MAX = (1 << 31) - 1
EDGES = (63, 64, 8191, 8192, 1048575, 1048576, 134217727, 134217728, I32_MAX)      # where a zigzag varint of an I32 grows by a byte, and its end
CRCS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
SIZES = (0, 1, 15, 16, 17, 65535, 65536, 65537, 1 << 20, 0x7E000000)


def fields(type=M.DATA_PAGE, usize=10, csize=10, crc=None, num_values=1, num_nulls=0, num_rows=0, encoding=0, def_enc=0, rep_enc=0, def_len=0, rep_len=0,
           is_compressed=True):
    v2 = type == M.DATA_PAGE_V2
    return dict(type=type, usize=usize, csize=csize, crc=crc or 0, has_crc=crc is not None, num_values=num_values, num_nulls=num_nulls if v2 else 0,
                num_rows=num_rows if v2 else 0, encoding=encoding, def_enc=def_enc if type == M.DATA_PAGE else 0, rep_enc=rep_enc if type == M.DATA_PAGE else 0,
                def_len=def_len if v2 else 0, rep_len=rep_len if v2 else 0, is_compressed=is_compressed if v2 else True)


def expected(f):
    """parquet_model.header() of the same fields"""
    return M.header(f["type"], f["usize"], f["csize"], f["crc"] if f["has_crc"] else None, num_values=f["num_values"], encoding=f["encoding"], def_enc=f["def_enc"],
                    rep_enc=f["rep_enc"], num_rows=f["num_rows"], num_nulls=f["num_nulls"], def_len=f["def_len"], rep_len=f["rep_len"],
                    is_compressed=f["is_compressed"] if f["type"] == M.DATA_PAGE_V2 else None)


def header_cases():
    cases = []
    for g in M.golden():                                        # every page of every golden chunk; num_nulls through the model's Reader
        code, pages = M.walk(g["chunk"])
        assert code == 0
        for pg, row in zip(pages, W.num_nulls(g["chunk"], g["pages"])):
            cases.append(fields(pg["type"], pg["usize"], pg["csize"], pg["crc"], pg["num_values"], row[0] >> 32, pg["num_rows"], pg["encoding"], pg["def_enc"],
                                pg["rep_enc"], pg["def_len"], pg["rep_len"], pg["is_compressed"]))
    assert any(c["num_nulls"] for c in cases) and {c["type"] for c in cases} == {0, 2, 3}
    for t in (M.DATA_PAGE, M.DICT_PAGE, M.DATA_PAGE_V2):
        for e in EDGES:
            cases += [fields(t, usize=e), fields(t, csize=e), fields(t, usize=e, csize=e, crc=e), fields(t, num_values=e), fields(t, num_values=-e), fields(t, num_values=-e - 1)]
        for crc in CRCS:
            cases += [fields(t, crc=crc), fields(t, usize=I32_MAX, csize=0, crc=crc)]
        for enc in (0, 63, 64, 255):
            cases.append(fields(t, encoding=enc, def_enc=255 - enc, rep_enc=enc ^ 64))
    for e in EDGES:                                             # V2's own fields; a level length needs both sizes at or above it
        big = dict(type=M.DATA_PAGE_V2, usize=I32_MAX, csize=I32_MAX)
        cases += [fields(**big, def_len=e), fields(**big, rep_len=e), fields(**big, def_len=e // 2, rep_len=e - e // 2), fields(M.DATA_PAGE_V2, num_nulls=e),
                  fields(M.DATA_PAGE_V2, num_rows=e), fields(M.DATA_PAGE_V2, num_nulls=-e - 1, num_rows=-e)]
    for flag in (True, False):
        cases += [fields(M.DATA_PAGE_V2, is_compressed=flag), fields(M.DATA_PAGE_V2, crc=5, def_len=3, rep_len=4, is_compressed=flag)]
    # the maximal header: every varint at its longest (an encoding has 8 bits; the two level lengths share the page's size)
    cases.append(fields(M.DATA_PAGE_V2, I32_MAX, I32_MAX, 0x7FFFFFFF, I32_MAX, I32_MAX, I32_MAX, 255, 0, 0, 1 << 30, (1 << 30) - 1, False))
    cases.append(fields(M.DATA_PAGE_V2, I32_MAX, I32_MAX, 0x80000000, -1 << 31, -1 << 31, -1 << 31, 255, 0, 0, (1 << 30) - 1, 1 << 30, True))
    return cases


def _words(f):
    return (C.c_longlong * len(WORDS))(*[int(f[k]) for k in WORDS])


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(build_sim("sim_parquet_write.cpp", str(tmp_path_factory.mktemp("parquet_write") / "libsim_parquet_write.so")))
    L.sim_pqw_read_back.restype = L.sim_pqw_row_fields.restype = C.c_longlong
    L.sim_pqw_read_back.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.sim_pqw_slot_bound.restype = L.sim_pqw_chunk_bound.restype = C.c_ulonglong
    L.sim_pqw_slot_bound.argtypes = [C.c_int, C.c_ulonglong]
    L.sim_pqw_chunk_bound.argtypes = [C.c_int, C.c_ulonglong, C.c_ulonglong]
    return L


def test_host_build_of_the_header_writer_against_the_model(sim):
    longest = 0
    cases = header_cases()
    assert len(cases) > 1000
    for f in cases:
        want = expected(f)
        w = _words(f)
        assert sim.sim_pqw_header_len(w) == len(want), f
        dst = C.create_string_buffer(b"\xa5" * 64, 64)
        assert sim.sim_pqw_write_header(w, dst) == len(want) and dst.raw[:len(want)] == want and dst.raw[len(want):] == b"\xa5" * (64 - len(want)), f
        back, used = (C.c_longlong * len(WORDS))(), C.c_ulonglong()
        assert sim.sim_pqw_read_back(want, len(want), back, C.byref(used)) == 0 and used.value == len(want), f
        assert dict(zip(WORDS, back)) == dict(f, num_nulls=0, has_crc=int(f["has_crc"]), is_compressed=int(f["is_compressed"])), f
        pg, end = M.page_header(want, 0)                        # ... and the reader's model
        assert end == len(want) and (pg["type"], pg["usize"], pg["csize"], pg["crc"]) == (f["type"], f["usize"], f["csize"], f["crc"] if f["has_crc"] else None)
        longest = max(longest, len(want))
    assert longest == sim.sim_pqw_max_header() == W.MAX_HEADER == 57


def test_header_writer_stand_alone_under_sanitizers(tmp_path):
    """a program of its own (SIM_MAIN), run directly: every header is written into a heap block of exactly its length"""
    assert SANITIZE
    exe = build_sim("sim_parquet_write.cpp", str(tmp_path / "sim_parquet_write_main"), main=True, sanitize=True)
    cases = header_cases()
    path = str(tmp_path / "parquet_write_cases.bin")
    with open(path, "wb") as out:
        out.write(struct.pack("<I", len(cases)))
        for f in cases:
            want = expected(f)
            out.write(struct.pack("<14q", *[int(f[k]) for k in WORDS]) + struct.pack("<I", len(want)) + want)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(cases) in r.stdout


def _row(r):
    return (C.c_longlong * 8)(*[W._i64(int(x)) for x in r])


def test_row_rules_of_the_host_build_are_the_models(sim):
    good = W.table_of([dict(type=3, usize=20, def_len=3, rep_len=4, num_values=7, num_rows=5, num_nulls=2, encoding=8, crc=True),
                       dict(type=0, usize=0, encoding=3, def_enc=3, rep_enc=4, crc=False), dict(type=2, usize=I32_MAX, num_values=-1)])
    bad = [[1] + good[0][1:], [4] + good[0][1:], [-1 & 0xFFFFFFFF] + good[0][1:], good[0][:3] + [-1] + good[0][4:], good[0][:3] + [1 << 31] + good[0][4:],
           good[1][:7] + [1], good[2][:7] + [1 << 32], good[0][:7] + [21], good[0][:7] + [10 | 11 << 32], good[0][:7] + [0xFFFFFFFF | 0xFFFFFFFF << 32]]
    for g in M.golden()[::5]:
        good += W.num_nulls(g["chunk"], g["pages"])
    for row in good + bad:
        w = (C.c_longlong * len(WORDS))()
        code, f = sim.sim_pqw_row_fields(_row(row), w), W.fields(row)
        assert (code == 0) == (f is not None) and code in (0, W.TABLE), row
        if f is not None:
            got = dict(zip(WORDS, w))
            assert all(got[k] == int(f[k]) for k in f), (row, got, f)
    assert all(W.fields(r) is None for r in bad) and all(W.fields(r) is not None for r in good)


def test_model_rules():
    rnd = random.Random(5)
    noise = bytes(rnd.randrange(256) for _ in range(64))
    data = b"ab" + b"c" * 40 + b"L" * 5 + noise + b"dict" * 4 + b"xyz"
    table = W.table_of([dict(type=0, usize=42, encoding=0, def_enc=3, rep_enc=3), dict(type=3, usize=69, def_len=2, rep_len=3, num_rows=4, num_nulls=1),
                        dict(type=2, usize=16, encoding=2, crc=False), dict(type=3, usize=3, def_len=3)])
    assert W.plan(table, len(data))[0] == 0 and [W.coded(f, "zstd") for f in W.plan(table, len(data))[1]] == [True, True, True, False]
    assert not any(W.coded(f, "uncompressed") for f in W.plan(table, len(data))[1])
    z = W.gz
    outs = [z(v) for _, v in W.values(table, data)]
    assert len(outs[1]) >= 64 and len(outs[2]) > 16              # noise does not shrink; neither do 16 bytes behind a gzip header
    res, chunk = W.write(table, data, "gzip", outs)
    code, pages = M.walk(chunk)
    assert code == 0 and res == len(chunk) and [p["type"] for p in pages] == [0, 3, 2, 3]
    # the choice rule: V2 raw with the flag false; V1 and dictionary pages carry the output even where it is longer
    assert [p["is_compressed"] for p in pages] == [True, False, True, False] and pages[1]["csize"] == pages[1]["usize"] == 69 and pages[2]["csize"] == len(outs[2])
    assert pages[3]["csize"] == 3 and (pages[1]["num_rows"], pages[1]["def_len"], pages[1]["rep_len"]) == (4, 2, 3)
    assert [p["crc"] is not None for p in pages] == [True, True, False, True]
    assert all(p["crc"] is None or p["crc"] == zlib.crc32(chunk[p["payload"]:p["payload"] + p["csize"]]) for p in pages)
    assert M.verdict(chunk, "gzip", len(data), verify_crc=True) == len(data)
    back = b"".join(chunk[p["payload"]:p["payload"] + p["def_len"] + p["rep_len"]] + (zlib.decompress(chunk[p["payload"] + p["def_len"] + p["rep_len"]:p["payload"] + p["csize"]], 31)
                    if M.coded(p, "gzip") else chunk[p["payload"] + p["def_len"] + p["rep_len"]:p["payload"] + p["csize"]]) for p in pages)
    assert back == data
    # the table the reader gives for the written chunk is the writer's, but for the offsets and bit 24
    for got, row in zip(M.table(pages), table):
        assert (got[0], got[3], got[5], got[7], got[6] & ~W.IS_COMPRESSED) == (row[0] & 0xFFFFFFFF, row[3], row[5], row[7], row[6] & ~W.IS_COMPRESSED)
    # a compressible V2 page: the output, flag true
    t2, d2 = W.table_of([dict(type=3, usize=405, def_len=5)]), b"LLLLL" + b"v" * 400
    res2, c2 = W.write(t2, d2, "gzip", [z(b"v" * 400)])
    assert M.walk(c2)[1][0]["is_compressed"] is True and M.walk(c2)[1][0]["csize"] == 5 + len(z(b"v" * 400)) < 405
    # an encoder's code: a V2 page falls back to the raw values, a V1 page gives it to the chunk — the first in page order
    assert W.write(t2, d2, "gzip", [-6])[0] == len(W.write(t2, d2, "uncompressed", [None])[1])
    assert W.write(table, data, "gzip", [outs[0], -6, -2, None])[0] == -2 and W.write(table, data, "gzip", [-6, -6, -2, None]) == (-6, b"")
    # uncompressed copies; the capacity is decided on the whole chunk
    resu, cu = W.write(table, data, "uncompressed", [None] * 4)
    assert M.verdict(cu, "uncompressed", len(data), verify_crc=True) == len(data) and W.write(table, data, "uncompressed", [None] * 4, cap=resu)[0] == resu
    assert W.write(table, data, "uncompressed", [None] * 4, cap=resu - 1) == (W.OUT_TOO_SMALL, b"")
    # the table's rules, in their order
    assert W.write([], b"", "zstd", []) == (0, b"") and W.write([], b"x", "zstd", [])[0] == W.TABLE
    assert W.plan(table, len(data) + 1)[0] == W.TABLE and W.plan(table[:3], len(data))[0] == W.TABLE
    assert W.plan(table, len(data), row_cnt=W.ROWS_MAX + 1)[0] == W.TABLE and W.plan(table, len(data), row_cnt=W.ROWS_MAX)[0] == 0
    assert W.plan([], W.IN_MAX + 1)[0] == W.INPUT_TOO_LARGE and W.plan([[1] + table[0][1:]], W.IN_MAX + 1)[0] == W.INPUT_TOO_LARGE
    assert W.plan([[7] + table[0][1:]] + table[1:], len(data))[0] == W.TABLE and W.plan(table[:1] + [table[1][:7] + [70]] + table[2:], len(data))[0] == W.TABLE
    assert W.with_crc(table, False)[0][6] & W.HAS_CRC == 0 and all(r[6] & W.HAS_CRC for r in W.with_crc(table, True))


def _inner_bound(L, codec, n):
    return {"snappy": lambda: L.cj_snappy_raw_max_compress_len(n), "gzip": lambda: L.cj_deflate_compress_bound(n, 2), "zstd": lambda: L.cj_zstd_compress_bound(n, 0),
            "lz4_raw": lambda: L.cj_lz4_block_compress_bound(n, 0), "uncompressed": lambda: n}[codec]()


def test_slot_bound_is_at_least_the_encoders_bound(sim):
    """cj::inner_bound is these four exports (cj_codecs.hpp); pure arithmetic, no device"""
    from cramjam_amd import _native as N
    L = N.lib()
    for codec, what in M.CODECS.items():
        for n in SIZES + tuple(range(0, 300)) + tuple(65536 * k + d for k in (1, 2, 3, 255, 256) for d in (-1, 0, 1)):
            inner = _inner_bound(L, codec, n)
            assert inner > 0 or n == 0, (codec, n)
            assert sim.sim_pqw_slot_bound(what, n) == W.slot_bound(codec, n) >= inner, (codec, n)
            assert W.slot_bound(codec, n) - inner <= 16, (codec, n)       # ... and no looser than a granule


def test_compress_bound_covers_every_cut(sim):
    from cramjam_amd import _native as N
    L = N.lib()
    rnd = random.Random(19)
    for codec, what in M.CODECS.items():
        assert L.cj_parquet_compress_bound(what, 0, 0) == 0 == W.bound(codec, 0, 0)
        assert L.cj_parquet_compress_bound(what, W.IN_MAX + 1, 1) == 0 and L.cj_parquet_compress_bound(what, 0, W.ROWS_MAX + 1) == 0
        assert L.cj_parquet_compress_bound(what, W.IN_MAX, 1) == W.bound(codec, W.IN_MAX, 1) > W.IN_MAX
        for trial in range(60):
            p = rnd.choice((1, 2, 3, 17, 64, 200))
            n = rnd.choice((0, 1, p, 1000, 65536, 65537, 262144 + 5, 3 * 65536, 1 << 20))
            cuts = sorted(rnd.randrange(n + 1) for _ in range(p - 1))
            sizes = [b - a for a, b in zip([0] + cuts, cuts + [n])]
            pages = []
            for s in sizes:                                     # the longest header a page of this size can have, and the levels anywhere
                t = rnd.choice((0, 2, 3))
                lv = rnd.randrange(s + 1) if t == 3 else 0
                pages.append(dict(type=t, usize=s, def_len=lv // 2, rep_len=lv - lv // 2, num_values=-1 << 31, num_rows=-1 << 31, num_nulls=-1 << 31, encoding=255,
                                  def_enc=255, rep_enc=255, crc=True))
            table = W.table_of(pages)
            # the worst the codec may do: an output as long as its bound (a V2 page then keeps its values: no shorter)
            outs = [bytes(_inner_bound(L, codec, f["usize"] - f["def_len"] - f["rep_len"])) for f in W.plan(table, n)[1]]
            res, _ = W.write(table, bytes(n), codec, outs)
            b = L.cj_parquet_compress_bound(what, n, p)
            assert 0 < res <= b == W.bound(codec, n, p) == sim.sim_pqw_chunk_bound(what, n, p), (codec, n, p, res, b)
    assert all(L.cj_parquet_compress_bound(w, 10, 1) == 0 for w in (3, 4, 5, 8, -1))
    # incompressible bytes through a real encoder: Python's zlib, gzip members
    for n, p in ((1, 1), (1000, 3), (65536, 1), (200000, 7)):
        data = bytes(rnd.randrange(256) for _ in range(n))
        for t in (0, 3):
            table = W.table_of([dict(type=t, usize=n // p + (n % p if k == 0 else 0)) for k in range(p)])
            res, chunk = W.write(table, data, "gzip", [W.gz(v) for _, v in W.values(table, data)])
            assert M.verdict(chunk, "gzip", n, verify_crc=True) == n and n < res <= L.cj_parquet_compress_bound(M.CODECS["gzip"], n, p)


def test_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    L = N.lib()
    p = C.c_void_p(64)                # (never dereferenced: the checks come first)
    nul = (None,) * 10
    for what in M.CODECS.values():
        assert L.cj_parquet_compress_device(None, what, 0, 0, *nul, None) == 0 and L.cj_parquet_compress_host(None, what, 0, 0, None, None, None, None, None, None, None) == 0
        assert L.cj_parquet_compress_device(None, what, 1, 0, *nul, None) == W.BAD_ARG and L.cj_parquet_compress_host(None, what, 2, 0, None, None, None, None, None, None, None) == W.BAD_ARG
        assert L.cj_parquet_compress_device(None, what, 1, 1, *([p] * 10), None) == W.BAD_ARG
        for k in range(10):           # a null row pointer, each of the ten
            assert L.cj_parquet_compress_device(None, what, 0, 1, *[None if j == k else p for j in range(10)], None) == W.BAD_ARG
        for k in range(7):
            assert L.cj_parquet_compress_host(None, what, 0, 1, *[None if j == k else p for j in range(7)]) == W.BAD_ARG
        assert L.cj_parquet_compress_device(None, what, 0, 0xFFFFFFF1, *([p] * 10), None) == W.BAD_ARG
        # the decoder's entries still take no compress
        assert L.cj_parquet_batch_device(None, what, N.OP_COMPRESS, 0, 0, None, None, None, None, None, None, None, None) == W.BAD_ARG
    for what in (3, 4, 5, 8, -1):
        assert L.cj_parquet_compress_device(None, what, 0, 0, *nul, None) == W.BAD_ARG and L.cj_parquet_compress_host(None, what, 0, 0, None, None, None, None, None, None, None) == W.BAD_ARG
    assert N.strerror(W.TABLE).startswith("parquet:") and N.E_PARQUET_TABLE == W.TABLE == -73
    assert L.cj_debug_parquet_slot_budget(0) == 256 << 20 and L.cj_debug_parquet_slot_budget(0) == 256 << 20
    for bad in ("lz4", "brotli", None, 2):
        with pytest.raises(ValueError):
            batch.parquet_compress_bound(bad, 1, 1)
        with pytest.raises(ValueError):
            batch.parquet_compress_chunks([b""], [[]], bad)
    assert batch.parquet_compress_bound("snappy", 600, 2) == W.bound("snappy", 600, 2) == 2 * (57 + 32) + 700
    with pytest.raises(ValueError):
        batch.parquet_compress_chunks([b""], [], "gzip")
