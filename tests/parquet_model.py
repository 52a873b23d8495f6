"""The model of Parquet column chunks, pure Python: the walk over the Thrift compact page headers with the rules of
cramjam_amd/csrc/parquet_grammar.hpp, the verdict rules of cj_parquet_batch_*, a header WRITER — so tests can frame golden page bodies
into chunks of any page count and shape —, and the golden chunks of tests/golden/golden_parquet* (pyarrow's writer;
make_golden_parquet.py).  No CPU codec is needed at test time: the decoded bytes of every golden page lie in the uncompressed file's
chunk of the same column, and the maker asserted that they are what the codecs give."""
import hashlib
import json
import os
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODECS = {"uncompressed": 0, "snappy": 1, "gzip": 2, "zstd": 6, "lz4_raw": 7}          # Parquet's CompressionCodec, by the names of cramjam_amd.batch
GOLDEN_NAME = {"uncompressed": "none", "snappy": "snappy", "gzip": "gzip", "zstd": "zstd", "lz4_raw": "lz4"}      # the names pyarrow's writer takes
REAL = ("snappy", "gzip", "zstd", "lz4_raw")
HEADER, SIZE, CRC, OUT_TOO_SMALL, BAD_ARG = -70, -71, -72, -6, -101
SKIP_DEPTH = 8
DATA_PAGE, INDEX_PAGE, DICT_PAGE, DATA_PAGE_V2 = 0, 1, 2, 3


class Malformed(Exception):
    pass


# ---- the compact protocol, read -------------------------------------------------------------------------------------------------------------
class Reader:
    def __init__(self, b, pos=0):
        self.b, self.pos = b, pos

    def byte(self):
        if self.pos >= len(self.b):
            raise Malformed("end")
        self.pos += 1
        return self.b[self.pos - 1]

    def varint(self):
        v = 0
        for k in range(10):
            x = self.byte()
            v |= (x & 0x7F) << (7 * k)
            if not x & 0x80:
                return v
        raise Malformed("varint of more than 10 bytes")

    def i32(self):
        v = self.varint()
        v = ((v >> 1) ^ -(v & 1)) & 0xFFFFFFFF
        return v - (1 << 32) if v >> 31 else v

    def size31(self):
        v = self.varint()
        if v > 0x7FFFFFFF:
            raise Malformed("size")
        return v

    def hop(self, k):
        if k > len(self.b) - self.pos:
            raise Malformed("end")
        self.pos += k

    def field(self, last):
        """(type, id); type 0 = stop"""
        x = self.byte()
        if x == 0:
            return 0, last
        t = x & 15
        if t == 0 or t > 12:
            raise Malformed("wire type")
        return (t, last + (x >> 4)) if x >> 4 else (t, self.i32())

    def skip(self, t, elem=False, depth=0):
        if t in (1, 2):
            if elem:
                self.hop(1)
        elif t == 3:
            self.hop(1)
        elif t in (4, 5, 6):
            self.varint()
        elif t == 7:
            self.hop(8)
        elif t == 8:
            self.hop(self.size31())
        elif t in (9, 10, 11, 12):
            if depth == SKIP_DEPTH:
                raise Malformed("nesting")
            if t == 12:
                last = 0
                while True:
                    ft, last = self.field(last)
                    if ft == 0:
                        break
                    self.skip(ft, False, depth + 1)
            elif t == 11:
                n = self.size31()
                kv = self.byte() if n else 0
                for _ in range(n):
                    self.skip(kv >> 4, True, depth + 1)
                    self.skip(kv & 15, True, depth + 1)
            else:
                x = self.byte()
                n = x >> 4
                if n == 15:
                    n = self.size31()
                for _ in range(n):
                    self.skip(x & 15, True, depth + 1)
        else:
            raise Malformed("wire type")

    def struct(self, want, required):
        """want: {id: 5 (an I32) or 1 (a bool)}; {id: value}, every id of `required` present"""
        out, last = {}, 0
        while True:
            t, last = self.field(last)
            if t == 0:
                break
            w = want.get(last)
            if w is None:
                self.skip(t)
            elif w == 1:
                if t not in (1, 2):
                    raise Malformed("wire type of a known field")
                out[last] = t == 1
            else:
                if t != w:
                    raise Malformed("wire type of a known field")
                out[last] = self.i32()
        if any(i not in out for i in required):
            raise Malformed("required field")
        return out


def page_header(b, pos):
    """(page dict, position behind the header) or Malformed.  The page: type, usize, csize, crc (None: none), num_values, num_rows,
    encoding, def_enc, rep_enc, def_len, rep_len, is_compressed"""
    r = Reader(b, pos)
    top, sub, last = {}, {}, 0
    while True:
        t, last = r.field(last)
        if t == 0:
            break
        if 1 <= last <= 4:
            if t != 5:
                raise Malformed("wire type of a known field")
            top[last] = r.i32()
        elif last in (5, 7, 8):
            if t != 12:
                raise Malformed("wire type of a known field")
            sub[last] = r.struct(*{5: ({1: 5, 2: 5, 3: 5, 4: 5}, (1, 2, 3, 4)), 7: ({1: 5, 2: 5}, (1, 2)),
                                   8: ({1: 5, 2: 5, 3: 5, 4: 5, 5: 5, 6: 5, 7: 1}, (1, 2, 3, 4, 5, 6))}[last])
        else:
            r.skip(t)
    if any(i not in top for i in (1, 2, 3)) or top[2] < 0 or top[3] < 0:
        raise Malformed("required field or negative size")
    pg = dict(type=top[1], usize=top[2], csize=top[3], crc=(top[4] & 0xFFFFFFFF) if 4 in top else None, num_values=0, num_rows=0, encoding=0, def_enc=0,
              rep_enc=0, def_len=0, rep_len=0, is_compressed=True)
    own = {DATA_PAGE: 5, DICT_PAGE: 7, DATA_PAGE_V2: 8}.get(pg["type"])
    if own is not None:
        if own not in sub:
            raise Malformed("the page type's struct")
        s = sub[own]
        if own == 5:
            pg.update(num_values=s[1], encoding=s[2], def_enc=s[3], rep_enc=s[4])
        elif own == 7:
            pg.update(num_values=s[1], encoding=s[2])
        else:
            pg.update(num_values=s[1], num_rows=s[3], encoding=s[4], def_len=s[5], rep_len=s[6], is_compressed=s.get(7, True))
            if s[5] < 0 or s[6] < 0 or s[5] + s[6] > pg["csize"] or s[5] + s[6] > pg["usize"]:
                raise Malformed("level lengths")
    return pg, r.pos


def skipped(pg):
    return pg["type"] not in (DATA_PAGE, DICT_PAGE, DATA_PAGE_V2)


def decoded(pg):
    return 0 if skipped(pg) else pg["usize"]


def walk(chunk):
    """(code, [page dicts with `payload`, the offset of the page's bytes]): 0 or HEADER, the pages before the error listed"""
    pages, p = [], 0
    while p < len(chunk):
        try:
            pg, q = page_header(chunk, p)
        except Malformed:
            return HEADER, pages
        if pg["csize"] > len(chunk) - q:
            return HEADER, pages
        pg["payload"] = q
        pages.append(pg)
        p = q + pg["csize"]
    return 0, pages


def u32(x):
    return x & 0xFFFFFFFF


def words(pg, out_at):
    """the eight words of the pages query"""
    return [pg["type"], pg["payload"], pg["csize"], pg["usize"], out_at, u32(pg["num_values"]) | u32(pg["num_rows"]) << 32,
            (pg["encoding"] & 0xFF) | (pg["def_enc"] & 0xFF) << 8 | (pg["rep_enc"] & 0xFF) << 16 | int(pg["is_compressed"]) << 24 | int(pg["crc"] is not None) << 25,
            u32(pg["def_len"]) | u32(pg["rep_len"]) << 32]


def table(pages):
    rows, at = [], 0
    for pg in pages:
        rows.append(words(pg, at))
        at += decoded(pg)
    return rows


def coded(pg, codec):
    """the codec is asked for this page's values"""
    lv = pg["def_len"] + pg["rep_len"]
    return not skipped(pg) and codec != "uncompressed" and pg["is_compressed"] and (pg["csize"] - lv, pg["usize"] - lv) != (0, 0)


def verdict(chunk, codec, cap=None, results=None, verify_crc=False):
    """The result of one chunk.  cap: the capacity (None: the size query).  results: per page the codec's result for its values where
    that is not the stated size (None elsewhere; looked at only for pages the codec is asked for).  Rules, in order: the walk's code;
    OUT_TOO_SMALL when the read pages' stated sizes' sum exceeds cap; the first page in page order with a code — CRC (verify_crc, a
    page with a crc that is not that of its payload), else the codec's negative result, else SIZE for a result below the stated size —;
    else the sum."""
    code, pages = walk(chunk)
    if code:
        return code
    total = sum(decoded(pg) for pg in pages)
    if cap is None:
        return total
    if total > cap:
        return OUT_TOO_SMALL
    for k, pg in enumerate(pages):
        if verify_crc and not skipped(pg) and pg["crc"] is not None and zlib.crc32(chunk[pg["payload"]:pg["payload"] + pg["csize"]]) != pg["crc"]:
            return CRC
        r = results[k] if results else None
        if r is not None and coded(pg, codec):
            stated = pg["usize"] - pg["def_len"] - pg["rep_len"]
            if r != stated:
                assert r < stated
                return r if r < 0 else SIZE
    return total


# ---- the compact protocol, written ----------------------------------------------------------------------------------------------------------
def wvarint(v):
    out = bytearray()
    while True:
        if v < 0x80:
            return bytes(out + bytes([v]))
        out.append((v & 0x7F) | 0x80)
        v >>= 7


def wzig(x):
    return wvarint(((x << 1) ^ (x >> 63)) & 0xFFFFFFFFFFFFFFFF)


class Struct:
    """a struct being written: fields in any order, short or long form"""

    def __init__(self):
        self.b, self.last = bytearray(), 0

    def head(self, fid, t, long_form=False):
        d = fid - self.last
        if 0 < d <= 15 and not long_form:
            self.b.append(d << 4 | t)
        else:
            self.b.append(t)
            self.b += wzig(fid)
        self.last = fid
        return self

    def i32(self, fid, v, long_form=False, t=5):
        self.head(fid, t, long_form)
        self.b += wzig(v)
        return self

    def boolean(self, fid, v):
        return self.head(fid, 1 if v else 2)

    def raw(self, fid, t, data, long_form=False):
        """a field of wire type t whose value bytes are given"""
        self.head(fid, t, long_form)
        self.b += data
        return self

    def sub(self, fid, s, long_form=False):
        return self.raw(fid, 12, s.end(), long_form)

    def end(self):
        return bytes(self.b) + b"\x00"


def header(type, usize, csize, crc=None, num_values=1, encoding=0, def_enc=3, rep_enc=3, num_rows=1, num_nulls=0, def_len=0, rep_len=0, is_compressed=None,
           extra=None, long_form=False, drop=(), sub_drop=(), own=None):
    """A PageHeader.  extra(struct): called on the PageHeader's struct before its page struct — adds unknown fields.  drop / sub_drop:
    field ids of the PageHeader / of the page's own struct that are left out.  own: the page struct's field id where it is not the
    type's (None with a type that has none: no struct)."""
    s = Struct()
    for fid, v in ((1, type), (2, usize), (3, csize)):
        if fid not in drop:
            s.i32(fid, v, long_form)
    if crc is not None:
        s.i32(4, crc - (1 << 32) if crc >> 31 else crc, long_form)
    if extra:
        extra(s)
    own = {DATA_PAGE: 5, DICT_PAGE: 7, DATA_PAGE_V2: 8}.get(type) if own is None else own
    if own is not None and own not in drop:
        d = Struct()
        fields = {5: ((1, num_values), (2, encoding), (3, def_enc), (4, rep_enc)), 7: ((1, num_values), (2, encoding)),
                  8: ((1, num_values), (2, num_nulls), (3, num_rows), (4, encoding), (5, def_len), (6, rep_len))}[own]
        for fid, v in fields:
            if fid not in sub_drop:
                d.i32(fid, v, long_form)
        if own == 8 and is_compressed is not None:
            d.boolean(7, is_compressed)
        s.sub(own, d, long_form)
    return s.end()


def page(body, usize, type=DATA_PAGE, crc=True, **kw):
    """header + body; crc: True — the body's own CRC —, an int, or None"""
    c = zlib.crc32(body) if crc is True else crc
    return header(type, usize, len(body), c, **kw) + bytes(body)


# ---- the golden chunks -------------------------------------------------------------------------------------------------------------------------
_golden = None


def golden():
    """[{name, codec (a GOLDEN_NAME value), what, version, chunk (bytes), pages [[8 words]], decoded_len, total_uncompressed_size, sha256}]"""
    global _golden
    if _golden is None:
        meta = json.load(open(os.path.join(GOLDEN, "golden_parquet.json")))
        bins = [open(os.path.join(GOLDEN, "golden_parquet_%d.bin" % k), "rb").read() for k in range(meta["bins"])]
        for r in meta["chunks"]:
            r["chunk"] = bins[r["bin"]][r["off"]:r["off"] + r["len"]]
        _golden = meta["chunks"]
    return _golden


def golden_of(codec, version=None, big=None):
    """the chunks of one codec (a CODECS name); big: only / without the files of the one large page"""
    return [g for g in golden() if g["codec"] == GOLDEN_NAME[codec] and version in (None, g["version"]) and big in (None, g["name"].startswith("big."))]


def plain_of(g):
    """the decoded bytes of golden chunk g: the page payloads of the uncompressed file's chunk of the same column, one after another"""
    name = g["name"].split(".")
    name[2] = "none"
    p = next(x for x in golden() if x["name"] == ".".join(name))
    return b"".join(p["chunk"][r[1]:r[1] + r[2]] for r in p["pages"])


def digest(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def bodies(codec, min_decoded=1, max_decoded=1 << 30, n=None):
    """(bytes as the codec wrote them, their decoded bytes) of golden V1 pages of one real codec, by decoded length: their whole payload
    is the codec's stream, so they frame as V1 pages or as the values of V2 pages"""
    out = []
    for g in golden_of(codec, 1):
        plain = plain_of(g)
        for r in g["pages"]:
            lv = (r[7] & 0xFFFFFFFF) + (r[7] >> 32)
            if lv == 0 and (r[6] >> 24) & 1 and min_decoded <= r[3] <= max_decoded:
                out.append((g["chunk"][r[1]:r[1] + r[2]], plain[r[4]:r[4] + r[3]]))
                if n is not None and len(out) == n:
                    return out
    return out
