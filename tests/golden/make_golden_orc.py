"""Writes tests/golden/golden_orc.bin + golden_orc.json: the compression streams of ORC files that pyarrow's ORC writer (the Apache ORC
C++ library) wrote — four codecs x compression block sizes 65 536 and 262 144 — as they lie in the files, with what they decode to.
Run on a machine with pyarrow; the tests need neither pyarrow nor any CPU codec.

Every stream is found with the minimal protobuf reader below (PostScript -> Footer -> StripeInformation -> StripeFooter -> Stream) and
decoded here chunk by chunk: ZLIB with zlib.decompress(c, -15), LZ4 with the pure-Python block decoder below, SNAPPY and ZSTD with
pyarrow's codecs at the length the chunk's own header states."""
import hashlib
import io
import json
import os
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc

HERE = os.path.dirname(os.path.abspath(__file__))
CODECS = {"zlib": 1, "snappy": 2, "lz4": 4, "zstd": 5}          # PostScript.compression
BLOCK_SIZES = (65536, 262144)
ROWS = 3000


def table():
    rng = np.random.default_rng(20240611)
    words = "stripe footer stream chunk header original compressed block codec column row index data length present dictionary".split()
    pool = [" ".join(rng.choice(words, 48)) + "." for _ in range(8)]
    text = [" ".join(pool[j] for j in rng.integers(0, len(pool), 1)) + " #%d" % i for i in range(ROWS)]      # ~340 bytes a row: 16 blocks of 64 KiB; few distinct sentences, or the LZ4 and Snappy files outgrow the fixture
    ints = np.cumsum(rng.integers(0, 50, ROWS)).astype(np.int64)
    return pa.table({"text": text, "n": ints, "x": rng.random(ROWS)})      # random doubles: incompressible, their chunks stay original


# ---- protobuf, as far as ORC's tail needs it ---------------------------------------------------------------------------------------------
def varint(b, p):
    v = s = 0
    while True:
        v |= (b[p] & 0x7F) << s
        s += 7
        p += 1
        if not b[p - 1] & 0x80:
            return v, p


def fields(b):
    """(field number, wire type, value) of a message; length-delimited values as bytes"""
    p, out = 0, []
    while p < len(b):
        key, p = varint(b, p)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, p = varint(b, p)
        elif wt == 2:
            n, p = varint(b, p)
            v, p = bytes(b[p:p + n]), p + n
        elif wt == 1:
            v, p = bytes(b[p:p + 8]), p + 8
        elif wt == 5:
            v, p = bytes(b[p:p + 4]), p + 4
        else:
            raise ValueError("wire type %d" % wt)
        out.append((f, wt, v))
    return out


def one(msg, f, default=0):
    return next((v for g, _, v in msg if g == f), default)


# ---- the chunks --------------------------------------------------------------------------------------------------------------------------
def lz4_block(src):
    out, p = bytearray(), 0
    while True:
        t = src[p]; p += 1
        n = t >> 4
        if n == 15:
            while True:
                n += src[p]; p += 1
                if src[p - 1] != 255:
                    break
        out += src[p:p + n]; p += n
        if p == len(src):
            return bytes(out)
        off = src[p] | src[p + 1] << 8; p += 2
        m = t & 15
        if m == 15:
            while True:
                m += src[p]; p += 1
                if src[p - 1] != 255:
                    break
        assert 0 < off <= len(out)
        for _ in range(m + 4):
            out.append(out[-off])


def zstd_content_size(c):
    assert c[:4] == b"\x28\xb5\x2f\xfd"
    fhd = c[4]
    single, p = (fhd >> 5) & 1, 5 + (0 if (fhd >> 5) & 1 else 1) + (0, 1, 2, 4)[fhd & 3]
    k = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    assert k, "the frame states no content size"
    return int.from_bytes(c[p:p + k], "little") + (256 if k == 2 else 0)


def decode_chunk(codec, c):
    if codec == "zlib":
        return zlib.decompress(c, -15)
    if codec == "lz4":
        return lz4_block(c)
    if codec == "snappy":
        return pa.Codec("snappy").decompress(c, decompressed_size=varint(c, 0)[0], asbytes=True)
    return pa.Codec("zstd").decompress(c, decompressed_size=zstd_content_size(c), asbytes=True)


def decode_stream(codec, block_size, s):
    """(decoded bytes, [(offset of the chunk's bytes, their length, original, decoded length, SHA-256 of the decoded bytes)])"""
    out, chunks, p = bytearray(), [], 0
    while p < len(s):
        h = int.from_bytes(s[p:p + 3], "little")
        n, orig = h >> 1, h & 1
        c = s[p + 3:p + 3 + n]
        assert len(c) == n
        d = c if orig else decode_chunk(codec, c)
        assert len(d) <= block_size
        chunks.append((p + 3, n, orig, len(d), hashlib.sha256(d).hexdigest()))
        out += d
        p += 3 + n
    return bytes(out), chunks


def streams_of(f):
    """(name, bytes) of every compression stream of the ORC file f, and (codec number, block size) from its PostScript"""
    ps_len = f[-1]
    ps = fields(f[-1 - ps_len:-1])
    footer_len, kind, block, meta_len = one(ps, 1), one(ps, 2), one(ps, 3), one(ps, 5)
    end = len(f) - 1 - ps_len
    footer = f[end - footer_len:end]
    meta = f[end - footer_len - meta_len:end - footer_len]
    out = []
    codec = next(k for k, v in CODECS.items() if v == kind)
    for si, (_, _, sb) in enumerate(x for x in fields(decode_stream(codec, block, footer)[0]) if x[0] == 3):
        info = fields(sb)
        off, ilen, dlen, flen = one(info, 1), one(info, 2), one(info, 3), one(info, 4)
        sfoot = f[off + ilen + dlen:off + ilen + dlen + flen]
        p = off
        for _, _, st in (x for x in fields(decode_stream(codec, block, sfoot)[0]) if x[0] == 1):
            m = fields(st)
            n = one(m, 3)
            out.append(("stripe%d.kind%d.col%d" % (si, one(m, 1), one(m, 2)), f[p:p + n]))
            p += n
        assert p == off + ilen + dlen
        out.append(("stripe%d.footer" % si, sfoot))
    if meta_len:
        out.append(("metadata", meta))
    out.append(("footer", footer))
    return out, kind, block


def main():
    t = table()
    blob, recs = bytearray(), []
    for codec in CODECS:
        for bs in BLOCK_SIZES:
            buf = io.BytesIO()
            orc.write_table(t, buf, compression=codec, compression_block_size=bs, compression_strategy="compression")     # ("speed": LZ4 stores every chunk)
            f = buf.getvalue()
            assert orc.read_table(io.BytesIO(f)).equals(t)
            streams, kind, block = streams_of(f)
            assert kind == CODECS[codec] and block == bs
            ncomp = norig = most = 0
            for name, s in streams:
                d, chunks = decode_stream(codec, bs, s)
                recs.append({"name": "%s.%d.%s" % (codec, bs, name), "codec": codec, "block_size": bs, "off": len(blob), "len": len(s),
                             "chunks": [list(c) for c in chunks], "decoded_len": len(d), "sha256": hashlib.sha256(d).hexdigest()})
                blob += s
                norig += sum(c[2] for c in chunks); ncomp += sum(1 - c[2] for c in chunks); most = max(most, len(chunks))
            # the fixture's condition: both kinds of chunk everywhere, a stream of 16 chunks or more at the small block size
            assert ncomp >= 1 and norig >= 1, (codec, bs, ncomp, norig)
            assert bs != 65536 or most >= 16, (codec, bs, most)
            print("%-6s %6d  file %7d bytes, %2d streams, %3d chunks, %2d original, longest stream %2d chunks" % (codec, bs, len(f), len(streams), ncomp + norig, norig, most))
    assert len(blob) < (1 << 20)
    open(os.path.join(HERE, "golden_orc.bin"), "wb").write(blob)
    json.dump({"streams": recs}, open(os.path.join(HERE, "golden_orc.json"), "w"), indent=0, separators=(",", ":"))
    print("%d streams, %d bytes" % (len(recs), len(blob)))


if __name__ == "__main__":
    main()
