"""Mint tests/golden/golden_blosc_zcodecs.json (one entry per line) and golden_blosc_zcodecs.bin (the chunks' bytes, back to back) from
c-blosc 1.x with cname = "zlib" and "zstd": valid chunks of seeded inputs (tests/blosc_zcodec_model.make_input: the inputs are
regenerated, not stored), malformed chunks made by seeded mutations INSIDE stream payloads and of stream words of four valid ones, the
header cases, and two hand-made chunks whose stream is a good zlib stream / Zstandard frame followed by one extra byte that the stream
word counts.  The verdict of every malformed and hand-made chunk is the model's (tests/blosc_zcodec_model.py: Python's zlib and
libzstd); what blosc_decompress_ctx returned for it is recorded beside it (`libblosc`: nbytes or a code <= 0), and
tests/test_blosc_zcodecs_model.py checks the two against each other where libblosc loads.  Loader and minting calls are
make_golden_blosc.py's.  Runs only where libblosc and libzstd load; no test runs it, test_blosc_zcodecs_model.py re-mints the valid chunks
to pin this script to the file."""
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import blosc_model as M  # noqa: E402
import blosc_zcodec_model as Z  # noqa: E402
import make_golden_blosc as G  # noqa: E402

CODECS = ("zlib", "zstd")
FORMAT = {"zlib": Z.FORMAT_ZLIB, "zstd": Z.FORMAT_ZSTD}


def recipes():
    out = []

    def add(cname, kind, size, typesize, filt, clevel=5, blocksize=0, split=4, seed=None):
        out.append(dict(kind=kind, size=size, typesize=typesize, filter=filt, clevel=clevel, cname=cname, blocksize=blocksize, split=split,
                        seed=len(out) + 1 if seed is None else seed))
    for cname in CODECS:
        # filter x typesize cells at 4 096 bytes (clevel and the data kind vary along them)
        for ti, ts in enumerate([1, 2, 4, 8, 16, 7]):
            for filt in (0, 1, 2):
                k = ti + filt
                add(cname, ["f32", "text", "i16", "f64"][k % 4], 4096, ts, filt, clevel=[1, 5, 9][k % 3])
        # split modes (always, never, forward-compatible) x clevel
        for split in (1, 2, 4):
            for clevel in (1, 5, 9):
                add(cname, "f32", 20000, 4, 1, clevel=clevel, split=split)
        add(cname, "rand", 100, 4, 1, clevel=0)                          # memcpyed
        add(cname, "zeros", 0, 4, 1)                                     # an empty chunk
        # 70 000 bytes in blocks of 8 192, unsplit: eight full blocks and a leftover block
        add(cname, "f32", 70000, 4, 1, blocksize=8192, split=2)
        add(cname, "text", 70000, 1, 0, blocksize=8192, split=2)
        add(cname, "i16", 70000, 2, 2, blocksize=8192, split=2)
        # ... and split: libblosc then takes typesize x the block size asked for and 64 KiB at least — one split block and a leftover
        # block, which is never split
        add(cname, "f32", 70000, 4, 1, blocksize=8192, split=1)
        add(cname, "f64", 70000, 8, 2, blocksize=8192, split=1)
        # 300 001 bytes as ONE stream (for Zstd: a frame of three blocks, the literal slot is used again)
        add(cname, "f32", 300001, 4, 1, blocksize=1 << 20, split=2)
        add(cname, "text", 300001, 1, 0, blocksize=1 << 20, split=2)
        # float32 with random low bytes behind the shuffle: one stream of a block is stored, its neighbours are not
        add(cname, "f32lo", 32768, 4, 1, split=1)
        add(cname, "f32lo", 40000, 4, 1, blocksize=8192, split=1)
        # noise: every stream stored (if libblosc does not write the chunk memcpyed)
        add(cname, "rand", 20000, 4, 1, split=1)
        add(cname, "rand", 20000, 1, 0)
        # direct streams (no transposition, no scratch): bitshuffle blocks whose element count is no multiple of 8, typesize 1 under shuffle
        add(cname, "f32", 4100, 4, 2, split=1)
        add(cname, "f64", 70004, 4, 2, blocksize=8212, split=1)
        add(cname, "text", 20000, 1, 1)
    return out


MUTATED = [("zlib", 4, 4096, 1), ("zlib", 8, 70000, 2), ("zstd", 2, 70000, 2), ("zstd", 4, 70000, 1)]       # (cname, typesize, size, filter) of the base chunks
PER_BASE = 75


def mutations(valid):
    """[(name, base index, mutation)]: a byte inside a compressed stream of the base chunk set to a seeded value or one bit of it
    flipped; a stream word + 1 or - 1 (- 1 on the last stream: a truncated last stream)"""
    import numpy as np
    import struct
    rng = np.random.default_rng(20263)
    out = []
    for cname, ts, size, filt in MUTATED:
        base = next(i for i, (r, _c) in enumerate(valid) if (r["cname"], r["typesize"], r["size"], r["filter"]) == (cname, ts, size, filt))
        chunk = valid[base][1]
        streams = Z.parse(chunk)[1]
        comp = [s for s in streams if not s[5]]
        assert comp, (cname, ts, size, filt)
        tag = "%s_t%d_s%d_f%d" % (cname, ts, size, filt)
        for k in range(PER_BASE):
            s = comp[int(rng.integers(0, len(comp)))]
            kind = k % 5
            if kind == 3:                                              # a stream word: the last stream's - 1, another one's + 1 or - 1
                if k % 10 == 3:
                    s, d = streams[-1], -1
                else:
                    s, d = streams[int(rng.integers(0, len(streams)))], (1 if k % 20 < 10 else -1)
                word = struct.unpack_from("<i", chunk, s[0] - 4)[0]
                out.append(("%s/word%d%+d" % (tag, s[0] - 4, d), base, ["put", s[0] - 4, "<i", word + d]))
                continue
            # the head of a stream (its headers), anywhere in it, its last bytes (checksum, last block), or one bit anywhere
            where = [int(rng.integers(0, min(s[1], 8))), int(rng.integers(0, s[1])), s[1] - 1 - int(rng.integers(0, min(s[1], 4))), 0, int(rng.integers(0, s[1]))][kind]
            off = s[0] + where
            val = chunk[off] ^ (1 << int(rng.integers(0, 8))) if kind == 4 else int(rng.integers(0, 256))
            if val == chunk[off]:
                val ^= 0x20
            out.append(("%s/byte%d=%d" % (tag, off, val), base, ["put", off, "<B", val]))
        c = chunk
        out.append((tag + "/versionlz2", base, ["put", 1, "<B", 2]))
        out.append((tag + "/format-snappy", base, ["put", 2, "<B", (c[2] & 31) | (2 << 5)]))
        out.append((tag + "/reserved-bit", base, ["put", 2, "<B", c[2] | 8]))
        out.append((tag + "/capacity-1", base, ["cut", len(c)]))       # the chunk as it is, into a capacity of nbytes - 1 (`cap`)
    return out


def hand_chunks():
    """[(name, bytes)]: a good stream followed by one extra byte, the stream word counting it"""
    import zstd_cases
    raw = M.make_input("text", 5000, 77)
    return [("zlib_stream_plus_one_byte", Z.wrap_one(Z.FORMAT_ZLIB, zlib.compress(raw, 6), len(raw), b"\0")),
            ("zstd_frame_plus_one_byte", Z.wrap_one(Z.FORMAT_ZSTD, zstd_cases.zstd_compress(raw, level=3), len(raw), b"\0"))]


def libblosc_version(L):
    L.blosc_get_version_string.restype = C.c_char_p
    return L.blosc_get_version_string().decode()


def libblosc_decode(L, chunk, cap):
    """blosc_decompress_ctx into a buffer of `cap` bytes: (return code, bytes).  The chunk is handed over with room behind it: libblosc
    takes the chunk's length from its header"""
    src = C.create_string_buffer(bytes(chunk) + bytes(64), len(chunk) + 64)
    dst = C.create_string_buffer(max(cap, 1))
    r = L.blosc_decompress_ctx(src, dst, cap, 1)
    return r, dst.raw[:max(r, 0)]


def build(L):
    version = libblosc_version(L)
    valid, blob, pairs = [], bytearray(), []
    for r in recipes():
        raw = Z.make_input(r["kind"], r["size"], r["seed"])
        chunk = G.mint(L, raw, r)
        assert (chunk[2] >> 5 == FORMAT[r["cname"]] or chunk[2] & 2 or not raw) and Z.decode(chunk) == raw, r
        valid.append(dict(recipe=r, nbytes=len(raw), sha256=hashlib.sha256(raw).hexdigest(), at=len(blob), len=len(chunk), libblosc_version=version))
        blob += chunk
        pairs.append((r, chunk))
    bad = []
    for name, base, mut in mutations(pairs):
        b = M.mutate(pairs[base][1], mut)
        cap = valid[base]["nbytes"] - (1 if name.endswith("/capacity-1") else 0)
        cls, out = Z.verdict(b, cap)
        e = dict(name=name, base=base, mutation=mut, verdict=cls, cap=cap)
        if cls == "ok":
            e.update(sha256=hashlib.sha256(out).hexdigest(), nbytes=len(out))
        e["libblosc"] = libblosc_decode(L, b, cap)[0]
        bad.append(e)
    hand = []
    for name, b in hand_chunks():
        nbytes = int.from_bytes(b[4:8], "little")
        cls, out = Z.verdict(b, nbytes)
        assert cls == M.CORRUPT, (name, cls)
        hand.append(dict(name=name, verdict=cls, cap=nbytes, at=len(blob), len=len(b), libblosc=libblosc_decode(L, b, nbytes)[0]))
        blob += b
    return dict(valid=valid, malformed=bad, hand=hand), bytes(blob)


if __name__ == "__main__":
    L = G.load_libblosc()
    if L is None:
        sys.exit("libblosc.so.1 not found")
    doc, blob = build(L)
    path = os.path.join(HERE, "golden_blosc_zcodecs.json")
    line = lambda e: json.dumps(e, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{" + ",".join('"%s":[\n%s\n]' % (k, ",\n".join(line(e) for e in doc[k])) for k in ("valid", "malformed", "hand")) + "}\n")
    with open(os.path.join(HERE, "golden_blosc_zcodecs.bin"), "wb") as f:
        f.write(blob)
    print(path, os.path.getsize(path), "bytes;", len(blob), "bytes of chunks;", len(doc["valid"]), "valid,", len(doc["malformed"]), "malformed,", len(doc["hand"]), "hand-made")
    print("libblosc disagrees on:", [(e["name"], e["verdict"], e["libblosc"]) for e in doc["malformed"] + doc["hand"] if (e["verdict"] == "ok") != (e["libblosc"] > 0)])
