"""The model of the Parquet writer, pure Python over tests/parquet_model.py: given a page table in the pages query's
layout, the decoded chunk and per page what the codec gave for its values, the chunk cj_parquet_compress_* writes and its result — the
table's rules in their order, the choice between the codec's output and the raw values, the empty values section, the CRC, the capacity,
and the bound.  The codec's output is an INPUT of the model: the GPU tests take it from the plain encoder batches."""
import zlib

import parquet_model as M

TABLE, INPUT_TOO_LARGE, COMPRESS_FAILED, OUT_TOO_SMALL, BAD_ARG = -73, -1, -2, M.OUT_TOO_SMALL, M.BAD_ARG
IN_MAX, ROWS_MAX = 0x7E000000, 0xFFFFFFF0
MAX_HEADER = 57
HAS_CRC, IS_COMPRESSED = 1 << 25, 1 << 24
# the encoders' bounds as v + g(v) + K (cramjam_hip.h: cj_parquet_compress_bound)
SLOT_EXTRA = {"uncompressed": lambda v: 0, "snappy": lambda v: v // 6, "gzip": lambda v: 10 * (v >> 16), "zstd": lambda v: 3 * (v >> 16), "lz4_raw": lambda v: v // 255}
SLOT_CONST = {"uncompressed": 0, "snappy": 32, "gzip": 23, "zstd": 13, "lz4_raw": 16}


def slot_bound(codec, v):
    return v + SLOT_EXTRA[codec](v) + SLOT_CONST[codec]


def bound(codec, n, pages):
    """cj_parquet_compress_bound"""
    if codec not in M.CODECS or n > IN_MAX or pages > ROWS_MAX:
        return 0
    return pages * (MAX_HEADER + SLOT_CONST[codec]) + n + SLOT_EXTRA[codec](n)


def gz(b):
    """a gzip member by Python's zlib"""
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(bytes(b)) + c.flush()


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def fields(row):
    """what the writer reads of a row, or None where the row is refused"""
    w = [_i64(int(x)) for x in row]
    t = _i32(w[0])
    if t not in (M.DATA_PAGE, M.DICT_PAGE, M.DATA_PAGE_V2) or not 0 <= w[3] <= 0x7FFFFFFF:
        return None
    d, r = w[7] & 0xFFFFFFFF, (w[7] >> 32) & 0xFFFFFFFF
    if (t != M.DATA_PAGE_V2 and w[7] != 0) or d + r > w[3]:
        return None
    v2 = t == M.DATA_PAGE_V2
    return dict(type=t, usize=w[3], num_values=_i32(w[5]), num_rows=_i32(w[5] >> 32) if v2 else 0, num_nulls=_i32(w[0] >> 32) if v2 else 0,
                encoding=w[6] & 0xFF, def_enc=(w[6] >> 8) & 0xFF, rep_enc=(w[6] >> 16) & 0xFF, def_len=d, rep_len=r, has_crc=bool(w[6] & HAS_CRC))


def plan(table, n, row_cnt=None):
    """(code, [fields]) — the table's rules in the writer's order"""
    if (len(table) if row_cnt is None else row_cnt) > ROWS_MAX:
        return TABLE, []
    if n > IN_MAX:
        return INPUT_TOO_LARGE, []
    pages = []
    for row in table:
        f = fields(row)
        if f is None:
            return TABLE, []
        pages.append(f)
    return (0 if sum(f["usize"] for f in pages) == n else TABLE), pages


def coded(f, codec):
    """the codec is asked for this page's values"""
    return codec != "uncompressed" and f["usize"] > f["def_len"] + f["rep_len"]


def values(table, data):
    """per page (the levels, the values) of a table that stands; what the encoders get is the values of the pages coded() names"""
    out, at = [], 0
    for f in plan(table, len(data))[1]:
        lv = f["def_len"] + f["rep_len"]
        out.append((bytes(data[at:at + lv]), bytes(data[at + lv:at + f["usize"]])))
        at += f["usize"]
    return out


def write(table, data, codec, outputs, cap=None, row_cnt=None):
    """(result, the chunk's bytes — b"" with a code).  outputs[k]: what the codec gave for page k's values — bytes, or its negative
    code — looked at only for the pages coded() names.  cap None: as much as it takes."""
    code, pages = plan(table, len(data), row_cnt)
    if code:
        return code, b""
    out = bytearray()
    for f, (levels, vals), o in zip(pages, values(table, data), outputs):
        comp = False
        if coded(f, codec):
            if f["type"] == M.DATA_PAGE_V2:
                comp = not isinstance(o, int) and 0 < len(o) < len(vals)
            elif isinstance(o, int) or len(o) == 0:
                return (o if isinstance(o, int) and o < 0 else COMPRESS_FAILED), b""
            else:
                comp = True
        body = levels + (bytes(o) if comp else vals)
        v2 = dict(num_rows=f["num_rows"], num_nulls=f["num_nulls"], def_len=f["def_len"], rep_len=f["rep_len"], is_compressed=comp) if f["type"] == M.DATA_PAGE_V2 else {}
        out += M.header(f["type"], f["usize"], len(body), zlib.crc32(body) if f["has_crc"] else None, num_values=f["num_values"], encoding=f["encoding"],
                        def_enc=f["def_enc"], rep_enc=f["rep_enc"], **v2) + body
    if cap is not None and len(out) > cap:
        return OUT_TOO_SMALL, b""
    return len(out), bytes(out)


def with_crc(table, on):
    return [list(r[:6]) + [(r[6] | HAS_CRC) if on else (r[6] & ~HAS_CRC)] + [r[7]] for r in table]


def num_nulls(chunk, table):
    """the table of a chunk as parquet_pages gives it, completed: V2's num_nulls, read from the chunk's headers, in the high half of word 0"""
    out, p = [], 0
    for row in table:
        row = list(row)
        if row[0] == M.DATA_PAGE_V2:
            r, last = M.Reader(chunk, p), 0
            while True:
                t, last = r.field(last)
                assert t != 0, "a V2 page without its struct"
                if last == 8:
                    s = r.struct({1: 5, 2: 5, 3: 5, 4: 5, 5: 5, 6: 5, 7: 1}, (1, 2, 3, 4, 5, 6))
                    row[0] |= (s[2] & 0xFFFFFFFF) << 32
                    break
                r.i32() if t == 5 else r.skip(t)
        out.append(row)
        p = row[1] + row[2]
    return out


def table_of(pages):
    """rows for the writer from page dicts: type, usize, and optionally num_values, num_rows, num_nulls, encoding, def_enc, rep_enc, def_len,
    rep_len, crc (bool)"""
    rows = []
    for pg in pages:
        g = lambda k, d=0: pg.get(k, d)
        rows.append([pg["type"] | (g("num_nulls") & 0xFFFFFFFF) << 32, 0, 0, pg["usize"], 0, (g("num_values", 1) & 0xFFFFFFFF) | (g("num_rows") & 0xFFFFFFFF) << 32,
                     g("encoding") | g("def_enc") << 8 | g("rep_enc") << 16 | (HAS_CRC if g("crc", True) else 0), g("def_len") | g("rep_len") << 32])
    return rows
