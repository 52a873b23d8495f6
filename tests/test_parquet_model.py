"""Parquet column chunks without a GPU: the fixture's conditions; the model's walk (tests/parquet_model.py) against the
page tables pyarrow's files gave; the host build of the walk (cramjam_amd/csrc/parquet_grammar.hpp, unchanged, tests/hostsim/
sim_parquet_grammar.cpp) against the model over every golden chunk, every single-byte truncation of a dozen pages' headers and the
header edges the grammar names, through ctypes and as a stand-alone program under AddressSanitizer and UBSan with every chunk flush
against the end of its allocation; the verdict rules; the argument checks that need no device."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

import parquet_model as M
from hostsim_build import SANITIZE, build_sim


def test_fixture_conditions():
    assert len(M.golden()) == 75
    for codec in M.CODECS:
        for version in (1, 2):
            gs = M.golden_of(codec, version, big=False)
            assert len(gs) == 7 and max(len(g["pages"]) for g in gs) >= 65, (codec, version)            # a chunk of at least 65 pages
            pages = [r for g in gs for r in g["pages"]]
            assert sum(r[0] == M.DICT_PAGE for r in pages) >= 1                                           # a dictionary page
            assert all((r[6] >> 25) & 1 for r in pages)                                                   # every page carries a CRC
            if version == 2:
                assert any((r[7] & 0xFFFFFFFF) and (r[7] >> 32) for r in pages)                           # both level sections non-empty
                assert any(r[0] == 3 and r[2] == (r[7] & 0xFFFFFFFF) + (r[7] >> 32) and r[3] == r[2] for r in pages)      # an empty values section
                if codec != "uncompressed":
                    flags = {(r[6] >> 24) & 1 for r in pages if r[0] == 3}
                    assert flags == {0, 1}, (codec, flags)                                                # both V2 flag values under a real codec
        big = M.golden_of(codec, big=True)
        assert len(big) == 1 and len(big[0]["pages"]) == 1 and big[0]["pages"][0][3] >= 100000
    for codec in M.REAL:        # what the GPU cases lean on: small V1 payloads of every codec, each the codec's stream from end to end
        assert len(M.bodies(codec, max_decoded=600)) >= 65, codec


def test_model_walk_gives_the_recorded_page_tables():
    for g in M.golden():
        code, pages = M.walk(g["chunk"])
        assert code == 0 and M.table(pages) == g["pages"], g["name"]
        assert sum(M.decoded(p) for p in pages) == g["decoded_len"] <= g["total_uncompressed_size"]
        assert g["total_uncompressed_size"] == g["decoded_len"] + sum(p["payload"] for p in pages) - sum(q["payload"] + q["csize"] for q in pages[:-1]), g["name"]
        for p in pages:
            assert zlib.crc32(g["chunk"][p["payload"]:p["payload"] + p["csize"]]) == p["crc"]
        plain = M.plain_of(g)
        assert M.digest(plain) == g["sha256"] and len(plain) == g["decoded_len"], g["name"]
        assert M.verdict(g["chunk"], "uncompressed") == g["decoded_len"] == M.verdict(g["chunk"], "uncompressed", g["decoded_len"], verify_crc=True)
        if g["codec"] == "gzip":                # the one codec Python reads
            out = b""
            for p in pages:
                lv = p["def_len"] + p["rep_len"]
                body = g["chunk"][p["payload"]:p["payload"] + p["csize"]]
                assert not p["is_compressed"] or M.coded(p, "gzip") == (len(body) > lv)
                out += body[:lv] + (zlib.decompress(body[lv:], 31) if M.coded(p, "gzip") else body[lv:])
            assert out == plain, g["name"]


# ---- header cases ---------------------------------------------------------------------------------------------------------------------------
BODY = b"0123456789"


def nested(depth):
    """the value of a struct field: `depth` structs inside one another, the innermost empty"""
    return b"\x1c" * (depth - 1) + b"\x00" * depth


def unknown_fields():
    """[(label, adds the field to a struct at id 9)] — one unknown field of each wire type, containers nested and long"""
    stats = M.Struct().raw(1, 8, b"\x03max").raw(2, 8, b"\x03min").i32(3, 7, t=6).i32(4, 9, t=6).raw(5, 8, b"\x00").boolean(7, True).boolean(8, False).end()
    deep = M.Struct().raw(1, 9, b"\x2c" + stats + M.Struct().raw(3, 11, b"\x02\x8c" + b"\x01k" + stats + b"\x00" + stats).end()).end()
    vals = [("true", 1, b""), ("false", 2, b""), ("byte", 3, b"\x7f"), ("i16", 4, b"\x81\x01"), ("i32", 5, b"\xff\xff\xff\xff\x0f"), ("i64", 6, b"\x80" * 9 + b"\x01"),
            ("double", 7, bytes(8)), ("binary", 8, b"\x05hello"), ("empty binary", 8, b"\x00"), ("list of i32", 9, b"\x35\x02\x04\x06"),
            ("long list of bytes", 9, b"\xf3\x14" + bytes(20)), ("set of bools", 10, b"\x32\x01\x02\x01"), ("list of binaries", 9, b"\x28\x01a\x00"),
            ("empty list", 9, b"\x05"), ("empty map", 11, b"\x00"), ("map i32 -> binary", 11, b"\x02\x58\x02\x01a\x04\x00"), ("map bool -> struct", 11, b"\x01\x1c\x01" + stats),
            ("struct", 12, stats), ("nested struct, list and map", 12, deep), ("nesting at the limit", 12, nested(M.SKIP_DEPTH))]
    return [(label, (lambda s, t=t, v=v: s.raw(9, t, v))) for label, t, v in vals]


def header_cases():
    """[(label, chunk, expected code, expected page count)] — reasoned, not measured: the model and the host build are both held to them"""
    ok, bad = lambda label, b, n=1: (label, b, 0, n), lambda label, b, n=0: (label, b, M.HEADER, n)
    v1 = lambda **kw: M.page(BODY, 10, **kw)
    v2 = lambda **kw: M.page(BODY, 10, type=M.DATA_PAGE_V2, **kw)
    cases = [ok("empty chunk", b"", 0), ok("v1", v1()), ok("dict", M.page(BODY, 10, type=M.DICT_PAGE)), ok("v2", v2(def_len=4, rep_len=6)),
             ok("v2 flag false", v2(is_compressed=False)), ok("long-form ids", v1(long_form=True)), ok("long-form ids v2", v2(long_form=True, def_len=1, is_compressed=True)),
             ok("no crc", v1(crc=None)), ok("two pages", v1() + v2(), 2), ok("usize 0", M.page(b"", 0)),
             ok("index page without a struct", M.page(BODY, 10, type=M.INDEX_PAGE)), ok("page type 7 with a V1 struct", M.page(BODY, 10, type=7, own=5)),
             bad("index page whose V2 struct lacks a field", M.page(BODY, 10, type=M.INDEX_PAGE, own=8, sub_drop=(3,))),
             bad("payload one byte past the end", v1()[:-1]), bad("second page's payload past the end", v1() + v1()[:-1], 1),
             bad("stop byte missing", v1()[:M.walk(v1())[1][0]["payload"] - 1]), bad("garbage behind the last page", v1() + b"\x00", 1)]
    for label, add in unknown_fields():
        cases.append(ok("unknown field in PageHeader: " + label, v1(extra=add)))
        # ... and inside the page's own struct, where Statistics stands: written by hand behind the known fields
        d = M.Struct().i32(1, 5).i32(2, 0).i32(3, 3).i32(4, 3)
        add(d)
        h = M.Struct().i32(1, 0).i32(2, 10).i32(3, 10).sub(5, d).end()
        cases.append(ok("unknown field in DataPageHeader: " + label, h + BODY))
    for t in (13, 14, 15):
        cases.append(bad("wire type %d" % t, v1(extra=lambda s, t=t: s.raw(9, t, b"\x00"))))
        cases.append(bad("list of wire type %d" % t, v1(extra=lambda s, t=t: s.raw(9, 9, bytes([0x10 | t, 0])))))
    cases += [bad("wire type 0 with a delta", v1(extra=lambda s: s.raw(9, 0, b""))),
              bad("nesting one past the limit", v1(extra=lambda s: s.raw(9, 12, nested(M.SKIP_DEPTH + 1)))),
              bad("lists one past the limit", v1(extra=lambda s: s.raw(9, 9, b"\x19" * M.SKIP_DEPTH + b"\x03"))),
              ok("lists at the limit", v1(extra=lambda s: s.raw(9, 9, b"\x19" * (M.SKIP_DEPTH - 1) + b"\x03"))),
              bad("11-byte varint", v1(extra=lambda s: s.raw(9, 6, b"\x80" * 10 + b"\x00"))),
              bad("11-byte varint in a known field", M.Struct().i32(1, 0).raw(2, 5, b"\x80" * 10 + b"\x00").i32(3, 10).sub(5, M.Struct().i32(1, 1).i32(2, 0).i32(3, 3).i32(4, 3)).end() + BODY),
              bad("binary past the end", v1(extra=lambda s: s.raw(9, 8, b"\xff\xff\x03"))), bad("binary length above 31 bits", v1(extra=lambda s: s.raw(9, 8, b"\x80\x80\x80\x80\x08"))),
              bad("list longer than the chunk", v1(extra=lambda s: s.raw(9, 9, b"\xf3\xff\xff\x03")))]
    # a 10-byte varint is taken, and an I32 is the low 32 bits of its zigzag value: 2^62 + 10 states 10
    ten = M.wvarint((1 << 63) | 20)
    assert len(ten) == 10
    cases.append(ok("10-byte varint", M.Struct().i32(1, 0).raw(2, 5, ten).i32(3, 10).sub(5, M.Struct().i32(1, 1).i32(2, 0).i32(3, 3).i32(4, 3)).end() + BODY))
    # required fields
    for fid in (1, 2, 3):
        cases.append(bad("PageHeader without field %d" % fid, v1(drop=(fid,))))
    cases += [bad("data page without its struct", v1(drop=(5,))), bad("dictionary page without its struct", M.page(BODY, 10, type=M.DICT_PAGE, drop=(7,))),
              bad("V2 page without its struct", v2(drop=(8,))), bad("data page with the V2 struct", v1(own=8)), bad("V2 page with the V1 struct", v2(own=5))]
    cases += [bad("DataPageHeader without field %d" % f, v1(sub_drop=(f,))) for f in (1, 2, 3, 4)]
    cases += [bad("DictionaryPageHeader without field %d" % f, M.page(BODY, 10, type=M.DICT_PAGE, sub_drop=(f,))) for f in (1, 2)]
    cases += [bad("DataPageHeaderV2 without field %d" % f, v2(sub_drop=(f,))) for f in (1, 2, 3, 4, 5, 6)]
    # sizes
    cases += [bad("negative uncompressed size", M.header(0, -1, 10) + BODY), bad("negative compressed size", M.header(0, 10, -1) + BODY),
              bad("negative definition length", v2(def_len=-1)), bad("negative repetition length", v2(rep_len=-1)),
              ok("levels fill the page", v2(def_len=3, rep_len=7)), bad("levels one above the compressed size", M.page(BODY, 12, type=M.DATA_PAGE_V2, def_len=5, rep_len=6)),
              bad("levels one above the uncompressed size", M.page(BODY, 9, type=M.DATA_PAGE_V2, def_len=10)), ok("sizes differ", M.page(BODY, 12, type=M.DATA_PAGE_V2, def_len=10))]
    # wire types of known fields
    wrong = lambda build: build.sub(5, M.Struct().i32(1, 1).i32(2, 0).i32(3, 3).i32(4, 3)).end() + BODY
    cases += [bad("type as an I64", wrong(M.Struct().i32(1, 0, t=6).i32(2, 10).i32(3, 10))), bad("size as an I16", wrong(M.Struct().i32(1, 0).i32(2, 10, t=4).i32(3, 10))),
              bad("crc as a binary", wrong(M.Struct().i32(1, 0).i32(2, 10).i32(3, 10).raw(4, 8, b"\x04abcd"))),
              bad("the page struct as a binary", M.Struct().i32(1, 0).i32(2, 10).i32(3, 10).raw(5, 8, b"\x00").end() + BODY),
              bad("num_values as a bool", M.Struct().i32(1, 0).i32(2, 10).i32(3, 10).sub(5, M.Struct().boolean(1, True).i32(2, 0).i32(3, 3).i32(4, 3)).end() + BODY)]
    v2s = lambda flag: M.Struct().i32(1, 1).i32(2, 0).i32(3, 1).i32(4, 0).i32(5, 0).i32(6, 0).raw(7, *flag)
    cases += [bad("is_compressed as an I32", M.Struct().i32(1, 3).i32(2, 10).i32(3, 10).sub(8, v2s((5, b"\x02"))).end() + BODY),
              ok("is_compressed true", M.Struct().i32(1, 3).i32(2, 10).i32(3, 10).sub(8, v2s((1, b""))).end() + BODY)]
    # a known id twice: the last one counts (the second, behind a higher id, has to take the long form)
    twice = M.Struct().i32(1, 0).i32(2, 99).i32(3, 10).i32(2, 10, long_form=True).sub(5, M.Struct().i32(1, 1).i32(2, 0).i32(3, 3).i32(4, 3).i32(1, 7, long_form=True)).end() + BODY
    cases.append(ok("fields twice", twice))
    return cases


def test_header_cases_by_the_model():
    seen = set()
    for label, b, code, npages in header_cases():
        got, pages = M.walk(b)
        assert (got, len(pages)) == (code, npages), label
        assert label not in seen
        seen.add(label)
    by = {c[0]: M.walk(c[1])[1] for c in header_cases()}
    assert by["10-byte varint"][0]["usize"] == 10 and by["fields twice"][0]["usize"] == 10 and by["fields twice"][0]["num_values"] == 7
    assert by["v2 flag false"][0]["is_compressed"] is False and by["v2"][0]["is_compressed"] is True and by["no crc"][0]["crc"] is None
    assert (by["v2"][0]["def_len"], by["v2"][0]["rep_len"]) == (4, 6) and by["long-form ids v2"][0]["def_len"] == 1
    assert M.decoded(by["index page without a struct"][0]) == 0 and M.skipped(by["page type 7 with a V1 struct"][0])


def walk_cases():
    """every golden chunk, every single-byte truncation of a dozen pages up to their payload, and the header cases"""
    cases = [g["chunk"] for g in M.golden()]
    dozen = [g for g in M.golden() if not g["name"].startswith("big.")][::6][:12]
    assert len(dozen) == 12 and {g["version"] for g in dozen} == {1, 2}
    for g in dozen:
        r = g["pages"][len(g["pages"]) // 2]
        start = g["pages"][len(g["pages"]) // 2 - 1][1] + g["pages"][len(g["pages"]) // 2 - 1][2] if len(g["pages"]) > 1 else 0
        page = g["chunk"][start:r[1] + r[2]]
        assert M.walk(page)[0] == 0
        cases += [page[:k] for k in range(r[1] - start + 2)] + [page[:-1]]
    return cases + [c[1] for c in header_cases()]


def test_model_walk_on_truncations():
    for b in walk_cases():
        code, pages = M.walk(b)
        end = pages[-1]["payload"] + pages[-1]["csize"] if pages else 0
        assert (code == 0) == (end == len(b)) and code in (0, M.HEADER) and len(pages) <= len(b)


def _rows(pages):
    return b"".join(struct.pack("<8q", *[w - (1 << 64) if w >> 63 else w for w in r]) for r in M.table(pages))


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(build_sim("sim_parquet_grammar.cpp", str(tmp_path_factory.mktemp("parquet") / "libsim_parquet_grammar.so")))
    L.sim_pq_walk.restype = C.c_longlong
    L.sim_pq_walk.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    return L


def test_host_build_of_the_walk_gives_the_models_verdict_and_pages(sim):
    assert sim.sim_pq_skip_depth() == M.SKIP_DEPTH >= 4
    for b in walk_cases():
        code, pages = M.walk(b)
        rows = (C.c_longlong * (8 * len(pages) + 8))()
        n = C.c_ulonglong()
        assert sim.sim_pq_walk(b, len(b), rows, len(pages) + 1, C.byref(n)) == code, b[:64]
        assert n.value == len(pages) and bytes(rows)[:64 * len(pages)] == _rows(pages)


def test_walk_stand_alone_under_sanitizers_on_every_case(tmp_path):
    """a program of its own (SIM_MAIN), run directly: every chunk is a heap block of exactly its size, so a read behind n ends it"""
    assert SANITIZE
    exe = build_sim("sim_parquet_grammar.cpp", str(tmp_path / "sim_parquet_grammar_main"), main=True, sanitize=True)
    cases = walk_cases()
    path = str(tmp_path / "parquet_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for b in cases:
            code, pages = M.walk(b)
            f.write(struct.pack("<IIq", len(b), len(pages), code) + b + _rows(pages))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(cases) in r.stdout


def test_verdict_rules():
    a, b = M.page(BODY, 10), M.page(BODY, 20)
    assert M.verdict(a + b, "zstd") == 30 and M.verdict(a + b, "zstd", 29) == M.OUT_TOO_SMALL and M.verdict(a + b, "zstd", 30) == 30
    assert M.verdict(a + b[:-1], "zstd", 0) == M.HEADER                                           # the walk first, then the capacity
    assert M.verdict(a + b, "zstd", 30, [None, 19]) == M.SIZE and M.verdict(a + b, "zstd", 30, [-51, 19]) == -51      # page order
    assert M.verdict(a + b, "uncompressed", 30, [-51, 19]) == 30                                  # a copied page has no result
    flipped = a + b[:-1] + b"X"
    assert M.verdict(flipped, "zstd", 30, verify_crc=True) == M.CRC and M.verdict(flipped, "zstd", 30) == 30
    assert M.verdict(flipped, "zstd", 30, [-51, None], verify_crc=True) == -51 and M.verdict(flipped, "zstd", 30, [None, -51], verify_crc=True) == M.CRC
    skip = M.page(BODY, 10, type=M.INDEX_PAGE, crc=1)
    assert M.verdict(a + skip + a, "zstd", 20, verify_crc=True) == 20 and M.verdict(a + skip + a, "zstd") == 20        # a skipped page: no room, no checksum
    v2 = M.page(BODY, 11, type=M.DATA_PAGE_V2, is_compressed=False)
    assert M.verdict(v2, "zstd", 11, [10]) == 11 and not M.coded(M.walk(v2)[1][0], "zstd")         # not the codec's: not checked for size
    assert not M.coded(M.walk(M.page(b"ab", 2, type=M.DATA_PAGE_V2, def_len=2))[1][0], "zstd")     # 0 bytes that state 0 bytes
    assert M.verdict(M.page(b"", 0, crc=5), "gzip", 0, verify_crc=True) == M.CRC and M.verdict(M.page(b"", 0, crc=0), "gzip", 0, verify_crc=True) == 0


def test_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = C.c_void_p(64)                # (never dereferenced: the checks come first)
    for what in M.CODECS.values():
        for flags in (0, N.PARQUET_FLAG_VERIFY_CRC):
            assert L.cj_parquet_batch_device(None, what, N.OP_DECOMPRESS, flags, 0, None, None, None, None, None, None, None, None) == 0
            assert L.cj_parquet_batch_host(None, what, N.OP_DECOMPRESS, flags, 0, None, None, None, None, None) == 0
        assert L.cj_parquet_batch_device(None, what, N.OP_COMPRESS, 0, 0, None, None, None, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_parquet_batch_host(None, what, N.OP_COMPRESS, 0, 0, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_parquet_batch_device(None, what, 2, 0, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
        assert L.cj_parquet_batch_device(None, what, N.OP_DECOMPRESS, 2, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
        assert L.cj_parquet_batch_device(None, what, N.OP_DECOMPRESS, 0, 1, p, p, p, None, p, p, p, None) == M.BAD_ARG      # a null row pointer
        assert L.cj_parquet_sizes_device(None, what, 0, 0, None, None, None, None, None) == 0 and L.cj_parquet_sizes_host(None, what, 0, 0, None, None, None) == 0
        assert L.cj_parquet_sizes_device(None, what, 1, 1, p, p, p, p, None) == M.BAD_ARG and L.cj_parquet_sizes_host(None, what, 1, 0, None, None, None) == M.BAD_ARG
        assert L.cj_parquet_sizes_device(None, what, 0, 1, p, p, None, p, None) == M.BAD_ARG
    for what in (3, 4, 5, 8, -1):     # LZO, BROTLI, the Hadoop-framed LZ4, nothing
        assert L.cj_parquet_batch_device(None, what, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_parquet_batch_host(None, what, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_parquet_sizes_host(None, what, 0, 0, None, None, None) == M.BAD_ARG and L.cj_parquet_sizes_device(None, what, 0, 0, None, None, None, None, None) == M.BAD_ARG
    assert L.cj_parquet_pages_device(None, 0, 0, None, None, None, None, None, None, None, None) == 0 and L.cj_parquet_pages_host(None, 0, 0, None, None, None, None, None) == 0
    assert L.cj_parquet_pages_device(None, 1, 0, None, None, None, None, None, None, None, None) == M.BAD_ARG and L.cj_parquet_pages_host(None, 1, 0, None, None, None, None, None) == M.BAD_ARG
    assert L.cj_parquet_pages_device(None, 0, 1, p, p, p, p, None, p, p, None) == M.BAD_ARG and L.cj_parquet_pages_device(None, 0, 1, p, p, p, p, p, None, p, None) == M.BAD_ARG
    assert L.cj_parquet_pages_device(None, 0, 1, p, p, p, None, None, None, None, None) == M.BAD_ARG and L.cj_parquet_pages_host(None, 0, 1, p, p, p, None, p) == M.BAD_ARG
    for code in (M.HEADER, M.SIZE, M.CRC):
        assert N.strerror(code).startswith("parquet:")
    assert (N.E_PARQUET_HEADER, N.E_PARQUET_SIZE, N.E_PARQUET_CRC) == (M.HEADER, M.SIZE, M.CRC) == (-70, -71, -72)
    assert {k: getattr(N, "PARQUET_" + k.upper()) for k in M.CODECS} == M.CODECS


def test_codec_names():
    from cramjam_amd import batch
    for bad in ("lz4", "lzo", "brotli", "none", "GZIP", None, 1):
        with pytest.raises(ValueError):
            batch.parquet_chunk_sizes([b""], bad)
        with pytest.raises(ValueError):
            batch.parquet_decompress_chunks([b""], bad, output_lens=[0])
        with pytest.raises(ValueError):
            batch.parquet_decompress_chunks_device(None, None, None, None, None, None, bad)
        with pytest.raises(ValueError):
            batch.parquet_chunk_sizes_device(None, None, None, bad)
