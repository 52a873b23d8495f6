"""The Parquet writer on the GPU (cj_parquet_compress_* / cramjam_amd.batch.parquet_compress_*), against the model of
tests/parquet_write_model.py byte for byte.  The codec's output is the model's input: it comes from the plain encoder batches
(lz4_compress_blocks, snappy_compress_raw_many, deflate_compress_many(wrapper="gzip"), zstd_compress_many) for the same values, so a
written chunk must be the model's chunk exactly.  What is written is then read back by the existing decoder with the CRCs verified, by
parquet_pages, and by the CPU: Python's zlib, the project's LZ4 and Snappy oracle, libzstd where the machine has it.  The device batches
go through the guarded harness of tests/device_batch.py: inputs at every misalignment with a neighbour's bytes behind them, 64 guard
bytes around every output slot, the result row filled with UNWRITTEN, a garbage row between the chunks' tables."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import device_batch as DB
import parquet_model as M
import parquet_write_model as W

pytestmark = pytest.mark.gpu
ALL = tuple(M.CODECS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GARBAGE = [0x7F7F7F7F7F7F7F7F] * 8        # the row in front of every chunk's table: read by nobody


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


# ---- the model's chunk ------------------------------------------------------------------------------------------------------------------------
_enc = {}


def encoded(codec, values):
    """what the codec's plain encoder batch gives for each of `values`: its bytes, or its negative code; one batch for all that are new"""
    from cramjam_amd import batch
    todo = [v for v in dict.fromkeys(values) if (codec, v) not in _enc]
    if todo:
        res, outs = {"lz4_raw": lambda: batch.lz4_compress_blocks(todo, store_size=False), "snappy": lambda: batch.snappy_compress_raw_many(todo),
                     "gzip": lambda: batch.deflate_compress_many(todo, wrapper="gzip"), "zstd": lambda: batch.zstd_compress_many(todo)}[codec]()
        for v, r, o in zip(todo, res, outs):
            _enc[(codec, v)] = bytes(o) if r > 0 else int(r)
    return [_enc[(codec, v)] for v in values]


def case(codec, table, data, cap=None, after=b"", **kw):
    """one chunk with the model's result and bytes; cap None: the bound"""
    fs, vals = W.plan(table, len(data), kw.get("row_cnt"))[1], W.values(table, data)
    outs = iter(encoded(codec, [v for f, (_, v) in zip(fs, vals) if W.coded(f, codec)]))
    cap = W.bound(codec, len(data), len(table)) if cap is None else cap
    res, out = W.write(table, data, codec, [next(outs) if W.coded(f, codec) else None for f in fs], cap, kw.get("row_cnt"))
    if "in_len" in kw:
        res, out = W.plan(table, kw["in_len"])[0], b""
        assert res < 0
    return dict(bytes=bytes(data), table=[list(r) for r in table], cap=cap, result=res, out=out, after=after, **kw)


def run_device(e, N, codec, cases, after=True):
    """one guarded device batch over the cases, held to the model's results and bytes and to the mask — nothing outside [0, result) of a
    written chunk, nothing at all for a refused one — with the input read back unchanged.  Returns (results, the written chunks)."""
    n, L, what = len(cases), N.lib(), M.CODECS[codec]
    blob, off, lens = DB.pack([c["bytes"] for c in cases], [c["after"] if after else b"" for c in cases])
    lens = np.array([c.get("in_len", l) for c, l in zip(cases, lens)], np.uint64)
    caps = np.array([c["cap"] for c in cases], np.uint64)
    want = np.array([c["result"] for c in cases], np.int64)
    ooff, total = DB.out_slots(caps, mis=DB.out_mis)
    rows, row_off = [], []
    for c in cases:
        rows.append(GARBAGE)
        row_off.append(len(rows))
        rows += c["table"]
    rows.append(GARBAGE)
    tab = np.array(rows, np.uint64).reshape(-1)
    row_cnt = [c.get("row_cnt", len(c["table"])) for c in cases]
    with DB.device_batch(e, blob, off, lens, ooff, caps, total, what=("parquet write", codec)) as b:
        d_in, p_off, p_len, d_out, p_ooff, p_cap, p_res = b.args
        d_tab = b.buffer(tab.nbytes)
        e.h2d(d_tab, tab)
        p_roff, p_rcnt = b.rows(row_off, row_cnt)
        N.check(L.cj_parquet_compress_device(e.h, what, 0, n, d_in, p_off, p_len, d_tab, p_roff, p_rcnt, d_out, p_ooff, p_cap, p_res, None))
        res, out, blob_after = b.read(with_input=True)
        assert (e.d2h(d_tab, tab.nbytes, "uint64") == tab).all(), "the tables were written"
    tag = lambda i: (codec, i, int(res[i]), int(want[i]), len(cases[i]["table"]))
    DB.check_results(res, want, tag)
    DB.check_mask(out, DB.untouched(ooff, want, total), ooff, tag)
    assert DB.guards_intact(out, ooff, caps) is None and (blob_after == blob).all()
    chunks = [out[int(o):int(o) + max(int(r), 0)].tobytes() for o, r in zip(ooff, res)]
    for i, c in enumerate(cases):
        assert chunks[i] == c["out"], ("bytes", tag(i))
    return [int(r) for r in res], chunks


def run_host(codec, cases, **kw):
    """the same cases through batch.parquet_compress_chunks (capacities: the bound)"""
    from cramjam_amd import batch
    res, chunks = batch.parquet_compress_chunks([c["bytes"] for c in cases], [c["table"] for c in cases], codec, **kw)
    assert list(res) == [c["result"] for c in cases], (codec, list(res)[:8])
    assert [bytes(x) for x in chunks] == [c["out"] for c in cases], codec
    return [bytes(x) for x in chunks]


def read_back(codec, cases, chunks):
    """the existing decoder with verify_crc gives the input back, and parquet_pages the input table but for the offsets and bit 24"""
    from cramjam_amd import batch
    ok = [k for k, c in enumerate(cases) if c["result"] >= 0]
    res, outs = batch.parquet_decompress_chunks([chunks[k] for k in ok], codec, output_lens=[len(cases[k]["bytes"]) for k in ok], verify_crc=True)
    assert list(res) == [len(cases[k]["bytes"]) for k in ok] and [bytes(o) for o in outs] == [cases[k]["bytes"] for k in ok], codec
    for k, t in zip(ok, batch.parquet_pages([chunks[k] for k in ok])):
        at = 0
        assert len(t) == len(cases[k]["table"])
        for got, row in zip(t.tolist(), cases[k]["table"]):
            f = W.fields(row)                                   # (num_rows and the level encodings exist only where the page type has them)
            w5 = (f["num_values"] & 0xFFFFFFFF) | (f["num_rows"] & 0xFFFFFFFF) << 32
            w6 = f["encoding"] | ((f["def_enc"] << 8 | f["rep_enc"] << 16) if f["type"] == M.DATA_PAGE else 0) | (W.HAS_CRC if f["has_crc"] else 0)
            assert (got[0], got[3], got[4], got[5], got[7], got[6] & ~W.IS_COMPRESSED) == (f["type"], row[3], at, w5, row[7], w6), (codec, k)
            at += row[3]


# ---- synthetic pages ------------------------------------------------------------------------------------------------------------------------------
_rnd = random.Random(0x5EED)
NOISE = bytes(_rnd.randrange(256) for _ in range(1 << 17))


def noise(k, n):
    at = (k * 7919) % (len(NOISE) - n)
    return NOISE[at:at + n]


def text(k, n):
    return ((b"page %d of the column, value after value; " % k) * (n // 20 + 1))[:n]


def chunk_of(pages):
    """pages: [(page dict for W.table_of without usize, the levels, the values)] -> (table, data)"""
    table = W.table_of([dict(p, usize=len(lv) + len(v), def_len=len(lv) // 2, rep_len=len(lv) - len(lv) // 2) for p, lv, v in pages])
    return table, b"".join(lv + v for _, lv, v in pages)


def mixed(n, base=0):
    """n pages of about 100 bytes: the three page types, text and noise, with and without levels and CRCs"""
    pages = []
    for k in range(base, base + n):
        t = (0, 3, 3, 2, 0)[k % 5]
        lv = bytes([k & 0xFF]) * (k % 7) if t == 3 else b""
        v = text(k, 90 + k % 23) if k % 3 else noise(k, 80 + k % 31)
        pages.append((dict(type=t, num_values=k, num_rows=k // 2, num_nulls=k % 3, encoding=k % 9, def_enc=3, rep_enc=4, crc=k % 4 != 1), lv, v))
    return chunk_of(pages)


# ---- the golden chunks ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    """every golden chunk decoded by the existing call, its table from parquet_pages completed with num_nulls: [(table, data)]"""
    from cramjam_amd import batch
    out = {}
    for codec in ALL:
        gs = M.golden_of(codec)
        res, outs = batch.parquet_decompress_chunks([g["chunk"] for g in gs], codec, output_lens=[g["decoded_len"] for g in gs], verify_crc=True)
        tabs = batch.parquet_pages([g["chunk"] for g in gs])
        for g, r, o, t in zip(gs, res, outs, tabs):
            assert r == g["decoded_len"] and M.digest(o) == g["sha256"]
            out[g["name"]] = (W.num_nulls(g["chunk"], t.tolist()), bytes(o))
    assert len(out) == 75
    return [out[g["name"]] for g in M.golden()]


_written = {}


def golden_written(golden, codec):
    if codec not in _written:
        cases = [case(codec, t, d) for t, d in golden]
        _written[codec] = cases, run_host(codec, cases)
    return _written[codec]


@pytest.mark.parametrize("codec", ALL)
def test_golden_chunks_host_and_device(eng, golden, codec):
    """each of the 75 decoded golden chunks written with this codec, as a host batch and as a device batch: the model's bytes; read back"""
    e, N = eng
    cases, chunks = golden_written(golden, codec)
    assert all(c["result"] > 0 for c in cases) and any(r[0] >> 32 for c in cases for r in c["table"])
    res, dev = run_device(e, N, codec, cases)
    assert dev == chunks
    read_back(codec, cases, chunks)
    if codec != "uncompressed":                                  # the fixture shows both outcomes of the choice
        flags = {p["is_compressed"] for x in chunks for p in M.walk(x)[1] if p["type"] == M.DATA_PAGE_V2}
        assert flags == {True, False}, (codec, flags)
        assert sum(len(x) for x in chunks) < sum(len(c["bytes"]) for c in cases)


def cpu_decoder(codec):
    """values -> bytes by a CPU library, or None where the machine has none"""
    import zlib
    if codec == "gzip":
        return lambda b, n: zlib.decompress(b, 31)
    if codec in ("snappy", "lz4_raw"):
        import oracle
        return (lambda b, n: oracle.snappy_decompress(b)[1]) if codec == "snappy" else (lambda b, n: oracle.lz4_decompress_raw(b, n)[1])
    try:
        import zstd_cases
        Z = zstd_cases.libzstd()
    except OSError:
        return None

    def dec(b, n):
        out = C.create_string_buffer(max(n, 1))
        r = Z.ZSTD_decompress(out, n, b, len(b))
        assert r == n, r
        return out.raw[:n]
    return dec


@pytest.mark.parametrize("codec", M.REAL)
def test_written_pages_are_read_by_the_cpu(eng, golden, codec):
    """every written page's values through a CPU decoder: Python's zlib, the LZ4 / Snappy oracle, libzstd"""
    dec = cpu_decoder(codec)
    if dec is None:
        pytest.skip("libzstd is not on this machine")
    cases, chunks = golden_written(golden, codec)
    seen = 0
    for c, x in zip(cases, chunks):
        code, pages = M.walk(x)
        assert code == 0
        at = 0
        for p in pages:
            lv = p["def_len"] + p["rep_len"]
            body = x[p["payload"]:p["payload"] + p["csize"]]
            vals = dec(body[lv:], p["usize"] - lv) if M.coded(p, codec) else body[lv:]
            seen += M.coded(p, codec)
            assert body[:lv] + vals == c["bytes"][at:at + p["usize"]], (codec, p)
            at += p["usize"]
    assert seen > 1000


# ---- page counts, level seams, page shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ALL)
def test_page_counts(eng, codec):
    """chunks of 0, 1, 63, 64, 65 and 130 pages in one batch: the layout's wave rounds; a neighbour's bytes behind every input or not"""
    e, N = eng
    cases = [case(codec, *mixed(n, 10 * n), after=noise(n, 40)) for n in (0, 1, 63, 64, 65, 130)]
    assert cases[0]["result"] == 0 and all(c["result"] > 0 for c in cases[1:])
    res, chunks = run_device(e, N, codec, cases)
    assert run_device(e, N, codec, cases, after=False) == (res, chunks)
    assert run_host(codec, cases) == chunks
    read_back(codec, cases, chunks)


@pytest.mark.parametrize("codec", ALL)
def test_v2_level_seams(eng, codec):
    """V2 pages whose levels are 0, 1, 3, 4, 5, 63, 64 and 65 bytes long in front of compressible and of random values: where the CRC
    passes from the levels in the input to the values in a slot or in the input"""
    e, N = eng
    pages = []
    for k, n in enumerate((0, 1, 3, 4, 5, 63, 64, 65)):
        lv = noise(100 + k, n)
        pages += [(dict(type=3, num_values=k, crc=True), lv, text(k, 300 + k)), (dict(type=3, num_values=k, crc=True), lv, noise(k, 97 + k))]
    cases = [case(codec, *chunk_of(pages), after=noise(1, 33))] + [case(codec, *chunk_of([p]), after=noise(2, 33)) for p in pages]
    res, chunks = run_device(e, N, codec, cases)
    read_back(codec, cases, chunks)
    flags = [p["is_compressed"] for p in M.walk(chunks[0])[1]]
    assert flags == ([True, False] * 8 if codec != "uncompressed" else [False] * 16)          # the choice rule: text shrinks, noise does not


@pytest.mark.parametrize("codec", M.REAL)
def test_choice_rule_and_page_shapes(eng, codec):
    """random values in a V2 page: raw, is_compressed false, both sizes equal; compressible ones: the output, true, smaller.  V1 and
    dictionary pages of random bytes carry the codec's output, longer than the values.  A values section of 0 bytes in each page type.
    One page of 120 000 bytes."""
    e, N = eng
    big = b"".join(text(k, 3000) + noise(k, 1000) for k in range(30))
    assert len(big) == 120000
    shapes = [(dict(type=3), b"ab", noise(1, 500)), (dict(type=3), b"ab", text(1, 500)), (dict(type=0), b"", noise(2, 500)), (dict(type=2), b"", noise(3, 500)),
              (dict(type=0), b"", b""), (dict(type=2), b"", b""), (dict(type=3), b"", b""), (dict(type=3), b"lvl", b""), (dict(type=0), b"", big)]
    cases = [case(codec, *chunk_of(shapes), after=noise(4, 20)), case(codec, *chunk_of([shapes[-1]])), case(codec, *chunk_of(shapes[4:8]))]
    res, chunks = run_device(e, N, codec, cases)
    assert run_host(codec, cases) == chunks
    read_back(codec, cases, chunks)
    p = M.walk(chunks[0])[1]
    assert (p[0]["is_compressed"], p[0]["csize"], p[0]["usize"]) == (False, 502, 502) and p[1]["is_compressed"] is True and p[1]["csize"] < p[1]["usize"] == 502
    assert p[2]["csize"] > 500 and p[3]["csize"] > 500 and [q["csize"] for q in p[4:8]] == [0, 0, 0, 3] and p[8]["csize"] < 120000
    assert [q["is_compressed"] for q in p[6:8]] == [False, False]


def test_crc_choice(eng):
    """rows with and without bit 25 in one chunk; write_crc True and False over the rows' own bits"""
    from cramjam_amd import batch
    e, N = eng
    table, data = mixed(20, 3)
    want = [bool(r[6] & W.HAS_CRC) for r in table]
    assert True in want and False in want
    for codec in ("zstd", "uncompressed"):
        res, chunks = run_device(e, N, codec, [case(codec, table, data)])
        assert [p["crc"] is not None for p in M.walk(chunks[0])[1]] == want
        for on in (True, False):
            c = case(codec, W.with_crc(table, on), data)
            got, = run_host(codec, [dict(c, table=table)], write_crc=on)
            assert got == c["out"] and [p["crc"] is not None for p in M.walk(got)[1]] == [on] * 20
        assert run_host(codec, [case(codec, table, data)], write_crc=None) == chunks
    out = bytearray(W.bound("zstd", len(data), 20) + 5)          # out=: views into one buffer
    res, views = batch.parquet_compress_chunks([data], [table], "zstd", out=out)
    want = case("zstd", table, data)["out"]
    assert res == [len(want)] and bytes(views[0]) == want == bytes(out[:res[0]])


@pytest.mark.parametrize("codec", ALL)
def test_capacities(eng, codec):
    """the bound suffices, the exact length suffices, one byte less is CJ_E_OUT_TOO_SMALL with the slot untouched"""
    e, N = eng
    base = [mixed(9, 1), mixed(65, 2), chunk_of([(dict(type=0), b"", noise(9, 3000))])]
    exact = [case(codec, t, d)["result"] for t, d in base]
    cases = [case(codec, t, d) for t, d in base] + [case(codec, t, d, cap=x) for (t, d), x in zip(base, exact)] + [case(codec, t, d, cap=x - 1) for (t, d), x in zip(base, exact)]
    cases.append(case(codec, *base[0], cap=0))
    assert [c["result"] for c in cases] == exact + exact + [W.OUT_TOO_SMALL] * 4
    run_device(e, N, codec, cases)


@pytest.mark.parametrize("codec", ("snappy", "gzip", "uncompressed"))
def test_table_errors(eng, codec):
    """each table error alone in a batch of good chunks: its code, its slot untouched, the neighbours as without it"""
    e, N = eng
    table, data = mixed(12, 5)
    v2 = next(k for k, r in enumerate(table) if r[0] & 0xFFFFFFFF == 3 and r[7])
    v1 = next(k for k, r in enumerate(table) if r[0] & 0xFFFFFFFF == 0)
    edit = lambda k, w, x: [list(r[:w]) + [x] + list(r[w + 1:]) if j == k else r for j, r in enumerate(table)]
    bad = [(edit(3, 0, 1), {}), (edit(3, 0, 7), {}), (edit(3, 0, 0xFFFFFFFF), {}), (edit(4, 3, (1 << 64) - 5), {}), (edit(4, 3, 1 << 31), {}),
           (edit(v1, 7, 1), {}), (edit(v1, 7, 1 << 32), {}), (edit(v2, 7, table[v2][3] + 1), {}), (edit(v2, 7, (table[v2][3] << 32) | 1), {}),
           (table[:-1], {}), (table + [table[0]], {}), (table, dict(row_cnt=0xFFFFFFF1)), (table, dict(in_len=0x7E000001)), ([], {})]
    good = case(codec, table, data, after=noise(7, 30))
    assert good["result"] > 0
    cases = []
    for t, kw in bad:
        cases += [good, case(codec, t, data, cap=good["cap"], **kw)]
    cases.append(good)
    want = [c["result"] for c in cases[1::2]]
    assert want == [W.TABLE] * 12 + [W.INPUT_TOO_LARGE, W.TABLE]
    res, chunks = run_device(e, N, codec, cases)
    assert set(chunks[0::2]) == {good["out"]}
    # the host entry: the same codes (a table of more rows than a batch can hold cannot be staged: refused before it is read)
    from cramjam_amd import batch
    host = [c for c in cases if "in_len" not in c and "row_cnt" not in c]
    hres, hchunks = batch.parquet_compress_chunks([c["bytes"] for c in host], [[[W._i64(x) for x in r] for r in c["table"]] for c in host], codec)
    assert list(hres) == [c["result"] for c in host] and [bytes(x) for x in hchunks] == [c["out"] for c in host]


# ---- turns, scratch, streams, far offsets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", M.REAL)
def test_turns(eng, codec):
    """three turns through cj_debug_parquet_slot_budget, plus a chunk larger than the budget: the one-turn bytes"""
    e, N = eng
    L = N.lib()
    big = chunk_of([(dict(type=0), b"", text(1, 50000) + noise(1, 10000))])
    cases = [case(codec, *mixed(10, 10 * k)) for k in range(5)] + [case(codec, *big), case(codec, *mixed(3, 70)), case(codec, [], b"")]
    one = run_device(e, N, codec, cases)
    slot = lambda c: sum((W.slot_bound(codec, f["usize"] - f["def_len"] - f["rep_len"]) + 15) // 16 * 16 for f in W.plan(c["table"], len(c["bytes"]))[1] if W.coded(f, codec))
    slots = [slot(c) for c in cases]
    budget = 2 * max(slots[:5])                                 # two small chunks a turn at most; the large one above it
    turns, fill = [[]], 0                                        # the host's cut: whole chunks, a new turn where the next one does not fit
    for k, x in enumerate(slots):
        if turns[-1] and fill + x > budget:
            turns.append([])
            fill = 0
        turns[-1].append(k)
        fill += x
    assert len(turns) >= 5 and [5] in turns and slots[5] > budget and max(len(t) for t in turns) >= 2, turns
    prev = L.cj_debug_parquet_slot_budget(budget)
    try:
        assert run_device(e, N, codec, cases) == one
        assert run_host(codec, cases) == one[1]
    finally:
        assert L.cj_debug_parquet_slot_budget(prev) == budget


def test_dirty_scratch(eng):
    """the same batch after other batches have used the engine's scratch, and after every scratch buffer was filled"""
    e, N = eng
    L = N.lib()
    cases = [case("gzip", *mixed(n, n)) for n in (1, 64, 65)] + [case("gzip", mixed(5, 1)[0][:-1], mixed(5, 1)[1])]
    other = [case("lz4_raw", *mixed(n, 3 * n)) for n in (130, 2)]
    first = run_device(e, N, "gzip", cases)
    run_device(e, N, "lz4_raw", other)
    run_device(e, N, "zstd", [case("zstd", *mixed(40, 9))])
    assert run_device(e, N, "gzip", cases) == first
    filled = (C.c_uint64 * L.cj_debug_scratch_count())()
    for pattern in (1, 2 + 0x5EED):
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        assert run_device(e, N, "gzip", cases) == first
        N.check(L.cj_debug_scratch_fill(e.h, pattern, filled))
        run_device(e, N, "lz4_raw", other)


def test_device_entry_on_torch_tensors():
    """parquet_compress_chunks_device on torch tensors on a side stream with sync=False, behind the decode and the pages query on the
    same stream, in a child that imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(ROOT, "tests", "parquet_write_torch_child.py"), "parquet write torch: ok", 600)


@pytest.mark.parametrize("codec", ("snappy", "zstd"))
def test_far_offsets(eng, golden, codec):
    """one batch placed beyond 4 GiB: both offset rows around 2^31 and 2^32 of two 6 GiB allocations"""
    e, N = eng
    L, what = N.lib(), M.CODECS[codec]
    small = [(t, d) for t, d in golden if 0 < len(d) <= 200000][::4][:14]
    cases = [case(codec, t, d) for t, d in small]
    cases += [dict(c, cap=c["result"] - 1, result=W.OUT_TOO_SMALL, out=b"") for c in cases[:2]]
    for c in cases:
        c["written"] = 0

    def call(idx, d_in, in_off, in_len, d_out, out_off, out_cap, result):
        rows, row_off = [], []
        for k in idx:
            rows.append(GARBAGE)
            row_off.append(len(rows))
            rows += cases[k]["table"]
        tab = np.array(rows, np.uint64).reshape(-1)
        b = DB._Batch(e, len(idx))
        try:
            d_tab = b.buffer(tab.nbytes)
            e.h2d(d_tab, tab)
            p_roff, p_rcnt = b.rows(row_off, [len(cases[k]["table"]) for k in idx])
            N.check(L.cj_parquet_compress_device(e.h, what, 0, len(idx), d_in, in_off, in_len, d_tab, p_roff, p_rcnt, d_out, out_off, out_cap, result, None))
            e.sync()
        finally:
            b.free()
    with DB.far_buffers(e, 32) as far:
        DB.run_far(e, far, "parquet-write-" + codec, cases, call, lambda i, got: (codec, "case", i, "got", got, "want", cases[i]["result"]))
