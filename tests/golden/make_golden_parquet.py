"""Writes tests/golden/golden_parquet_<k>.bin + golden_parquet.json: the column chunks of Parquet files that pyarrow's writer (the Apache
Parquet C++ library) wrote — five codecs x both data page versions, with page checksums — as they lie in the files, with their page
tables and what they decode to.  Run on a machine with pyarrow; the tests need neither pyarrow nor any CPU codec.

The chunks are found through pyarrow's view of the footer; their pages with the minimal Thrift compact reader below, decoded here page by
page with pa.Codec, every CRC checked with zlib.crc32.  The decoded chunk of every compressed file must equal the same chunk of the
uncompressed file, so the tests have every page's decoded bytes without a codec: they lie in the `none` file."""
import hashlib
import io
import json
import os
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

HERE = os.path.dirname(os.path.abspath(__file__))
CODECS = {"none": 0, "snappy": 1, "gzip": 2, "zstd": 6, "lz4": 7}      # CompressionCodec as the tests pass it: pyarrow's "lz4" writes raw blocks (LZ4_RAW)
PA_CODEC = {"snappy": "snappy", "gzip": "gzip", "zstd": "zstd", "lz4": "lz4_raw"}
ROWS = 3000
BIN_MAX = 1000000               # bytes per .bin file: below the repository's limit for a committed file


def table():
    rng = np.random.default_rng(20250309)
    words = "page header chunk column values levels repetition definition dictionary checksum codec footer offset length row group".split()
    text = [" ".join(rng.choice(words, 6)) + " #%d" % i for i in range(ROWS)]
    some = rng.random(ROWS) < 0.8
    lists = [None if r < 0.15 else [int(x) for x in rng.integers(0, 1000, int(rng.integers(0, 4)))] for r in rng.random(ROWS)]
    return pa.table({
        "ramp": pa.array(np.arange(ROWS, dtype=np.int64) * 3 + 7),
        "text": pa.array(text),
        "word": pa.array([words[j] for j in rng.integers(0, len(words), ROWS)]),
        "x": pa.array(rng.random(ROWS)),
        "maybe": pa.array(np.where(some, rng.integers(0, 100, ROWS), 0).astype(np.int32), mask=~some),
        "nothing": pa.array([None] * ROWS, pa.int32()),
        "list": pa.array(lists, pa.list_(pa.int32())),
    })


def big_table():
    """one compressible column whose single page decodes to at least 100 000 bytes"""
    rng = np.random.default_rng(77)
    words = "the quick brown fox jumps over the lazy dog and runs far away from here".split()
    return pa.table({"big": pa.array([" ".join(rng.choice(words, 9)) for _ in range(2600)])})


# ---- Thrift's compact protocol, as far as a PageHeader needs it ----------------------------------------------------------------------------
def varint(b, p):
    v = s = 0
    while True:
        v |= (b[p] & 0x7F) << s
        s += 7
        p += 1
        if not b[p - 1] & 0x80:
            return v, p


def zigzag(v):
    return (v >> 1) ^ -(v & 1)


def value(b, p, t, elem=False):
    if t in (1, 2):
        return (b[p] == 1, p + 1) if elem else (t == 1, p)
    if t == 3:
        return b[p], p + 1
    if t in (4, 5, 6):
        v, p = varint(b, p)
        return zigzag(v), p
    if t == 7:
        return bytes(b[p:p + 8]), p + 8
    if t == 8:
        n, p = varint(b, p)
        return bytes(b[p:p + n]), p + n
    if t in (9, 10):
        n, et = b[p] >> 4, b[p] & 15
        p += 1
        if n == 15:
            n, p = varint(b, p)
        out = []
        for _ in range(n):
            v, p = value(b, p, et, True)
            out.append(v)
        return out, p
    if t == 12:
        return struct(b, p)
    raise ValueError("compact type %d" % t)


def struct(b, p):
    """({field id: value}, position behind the stop byte)"""
    out, fid = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        if h >> 4:
            fid += h >> 4
        else:
            v, p = varint(b, p)
            fid = zigzag(v)
        out[fid], p = value(b, p, h & 15)


def pages_of(chunk, codec):
    """(decoded chunk, [the eight words of every page]) — every CRC checked"""
    out, rows, p = bytearray(), [], 0
    while p < len(chunk):
        h, q = struct(chunk, p)
        ptype, usize, csize = h[1], h[2], h[3]
        payload = chunk[q:q + csize]
        assert len(payload) == csize and 4 in h, "every page carries a CRC"
        assert zlib.crc32(payload) == h[4] & 0xFFFFFFFF
        nv = nr = enc = denc = renc = dl = rl = 0
        comp = True
        if ptype == 0:
            nv, enc, denc, renc = h[5][1], h[5][2], h[5][3], h[5][4]
        elif ptype == 2:
            nv, enc = h[7][1], h[7][2]
        elif ptype == 3:
            d = h[8]
            nv, nr, enc, dl, rl, comp = d[1], d[3], d[4], d[5], d[6], d.get(7, True)
        else:
            raise ValueError("page type %d" % ptype)
        lv = dl + rl
        vals = payload[lv:]
        if codec != "none" and comp and not (len(vals) == 0 and usize == lv):
            vals = pa.Codec(PA_CODEC[codec]).decompress(vals, decompressed_size=usize - lv, asbytes=True)
        assert len(vals) == usize - lv
        rows.append([ptype, q, csize, usize, len(out), nv | nr << 32, enc | denc << 8 | renc << 16 | int(comp) << 24 | 1 << 25, dl | rl << 32])
        out += payload[:lv] + vals
        p = q + csize
    assert p == len(chunk), "the pages tile the chunk"
    return bytes(out), rows


def chunks_of(f):
    """(column name, offset, length, total_uncompressed_size) of every column chunk of the file's one row group"""
    md = pq.ParquetFile(io.BytesIO(f)).metadata
    assert md.num_row_groups == 1
    rg = md.row_group(0)
    out = []
    for j in range(rg.num_columns):
        c = rg.column(j)
        start = c.dictionary_page_offset if c.has_dictionary_page else c.data_page_offset
        out.append((c.path_in_schema, start, c.total_compressed_size, c.total_uncompressed_size))
    return out


def main():
    blobs, recs, plain = [bytearray()], [], {}

    def add(name, codec, version, f):
        stats = dict(pages=0, most=0, dict=0, both=0, empty=0, comp=[0, 0])
        for col, off, n, total_u in chunks_of(f):
            chunk = f[off:off + n]
            decoded, rows = pages_of(chunk, codec)
            assert len(decoded) <= total_u, "the footer's size is an upper bound"
            key = (name.split(".")[0], version, col)
            if codec == "none":
                plain[key] = decoded
            else:
                assert plain[key] == decoded, ("the compressed file's chunk decodes to the uncompressed file's", name, col)
            if len(blobs[-1]) + n > BIN_MAX:
                blobs.append(bytearray())
            recs.append({"name": "%s.%s" % (name, col), "codec": codec, "what": CODECS[codec], "version": version, "bin": len(blobs) - 1, "off": len(blobs[-1]),
                         "len": n, "pages": rows, "decoded_len": len(decoded), "total_uncompressed_size": total_u, "sha256": hashlib.sha256(decoded).hexdigest()})
            blobs[-1] += chunk
            stats["pages"] += len(rows); stats["most"] = max(stats["most"], len(rows))
            for r in rows:
                stats["dict"] += r[0] == 2
                stats["both"] += r[0] == 3 and (r[7] & 0xFFFFFFFF) > 0 and (r[7] >> 32) > 0
                stats["empty"] += r[0] == 3 and r[2] == (r[7] & 0xFFFFFFFF) + (r[7] >> 32)
                if r[0] == 3:
                    stats["comp"][(r[6] >> 24) & 1] += 1
        print("%-18s file %7d bytes, %4d pages, longest chunk %3d, %d dictionary, %3d V2 with both levels, %d empty values, V2 is_compressed false/true %s"
              % (name, len(f), stats["pages"], stats["most"], stats["dict"], stats["both"], stats["empty"], stats["comp"]))
        return stats

    t, big = table(), big_table()
    for version in ("1.0", "2.0"):
        for codec in CODECS:
            buf = io.BytesIO()
            pq.write_table(t, buf, compression=codec, data_page_version=version, data_page_size=512, write_batch_size=32, write_page_checksum=True,
                           use_dictionary=["word"], row_group_size=ROWS)
            f = buf.getvalue()
            assert pq.read_table(io.BytesIO(f)).equals(t)
            s = add("table.v%s.%s" % (version[0], codec), codec, int(version[0]), f)
            # the fixture's conditions
            assert s["most"] >= 65 and s["dict"] >= 1, s
            if version == "2.0":
                assert s["both"] >= 1 and s["empty"] >= 1, s
                if codec in ("snappy", "lz4"):
                    assert s["comp"][0] >= 1 and s["comp"][1] >= 1, s
    for codec in CODECS:
        buf = io.BytesIO()
        pq.write_table(big, buf, compression=codec, data_page_version="1.0", data_page_size=1 << 20, write_page_checksum=True, use_dictionary=False)
        f = buf.getvalue()
        add("big.v1.%s" % codec, codec, 1, f)
        assert len(recs[-1]["pages"]) == 1 and recs[-1]["pages"][0][3] >= 100000
        if codec == "lz4":      # pyarrow's metadata prints LZ4 for raw blocks too: the flavour is what decodes them
            r = recs[-1]
            body = bytes(blobs[r["bin"]][r["off"] + r["pages"][0][1]:r["off"] + r["len"]])
            assert hashlib.sha256(pa.Codec("lz4_raw").decompress(body, decompressed_size=r["decoded_len"], asbytes=True)).hexdigest() == r["sha256"]
    for k, b in enumerate(blobs):
        assert len(b) < (1 << 20)
        open(os.path.join(HERE, "golden_parquet_%d.bin" % k), "wb").write(b)
    json.dump({"bins": len(blobs), "chunks": recs}, open(os.path.join(HERE, "golden_parquet.json"), "w"), indent=0, separators=(",", ":"))
    print("%d chunks, %d bytes in %d files" % (len(recs), sum(len(b) for b in blobs), len(blobs)))


if __name__ == "__main__":
    main()
