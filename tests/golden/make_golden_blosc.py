"""Mint tests/golden/golden_blosc.json (one entry per line) and golden_blosc.bin (the chunks' bytes, back to back) from c-blosc 1.x (libblosc.so.1 next to the Python interpreter's libraries): valid chunks of
seeded inputs (tests/blosc_model.make_input: the inputs are regenerated, not stored) and malformed chunks made by seeded mutation
of valid ones, whose expected verdict is the MODEL's (tests/blosc_model.py) — mutated chunks are never handed to libblosc's
decoder, which trusts its header in places; blosc_cbuffer_validate's answer is recorded beside the verdict for information.
The issue's matrix (typesize x size x filter x clevel x blocksize x codec, 3 240 cells) is SAMPLED: every typesize x size x filter cell
is there, clevel / blocksize / codec vary along it, so that the chunks stay within 1 MiB; and the bytes lie in a binary file beside
the JSON index rather than as base64 inside it (a readable diff).  Runs only where libblosc loads; no test runs it, tests/test_blosc_model.py re-mints the valid chunks to pin this script to the file."""
import ctypes as C
import glob
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import blosc_model as M  # noqa: E402


def load_libblosc():
    """c-blosc 1.x: $LIBBLOSC, or libblosc.so.1 under the interpreter's prefix, a conda prefix or the system's library directories"""
    pats = [os.environ.get("LIBBLOSC", ""), os.path.join(sys.prefix, "lib", "libblosc.so.1"), os.path.join(os.environ.get("CONDA_PREFIX", "/opt/conda"), "lib", "libblosc.so.1"),
            "/usr/lib/*/libblosc.so.1", "/usr/lib64/libblosc.so.1", "/usr/local/lib/libblosc.so.1"]
    for pat in pats:
        for p in sorted(glob.glob(pat)) if pat else []:
            try:
                L = C.CDLL(p)
            except OSError:
                continue
            L.blosc_compress_ctx.restype = C.c_int
            L.blosc_compress_ctx.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
            L.blosc_decompress_ctx.restype = C.c_int
            L.blosc_decompress_ctx.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            L.blosc_cbuffer_validate.restype = C.c_int
            L.blosc_cbuffer_validate.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            L.blosc_set_splitmode.argtypes = [C.c_int]
            return L
    return None


def mint(L, raw, p):
    """one chunk by the recipe p (dict: typesize, filter, clevel, cname, blocksize, split)"""
    L.blosc_set_splitmode(p["split"])
    cap = len(raw) + 1024
    dst = C.create_string_buffer(cap)
    r = L.blosc_compress_ctx(p["clevel"], p["filter"], p["typesize"], len(raw), raw, dst, cap, p["cname"].encode(), p["blocksize"], 1)
    L.blosc_set_splitmode(4)
    assert r > 0, (r, p)
    return dst.raw[:r]


def validate(L, chunk):
    n = C.c_size_t(0)
    return L.blosc_cbuffer_validate(chunk, len(chunk), C.byref(n))


def recipes():
    out = []

    def add(kind, size, typesize, filt, clevel=5, cname="lz4", blocksize=0, split=4, seed=None):
        out.append(dict(kind=kind, size=size, typesize=typesize, filter=filt, clevel=clevel, cname=cname, blocksize=blocksize, split=split,
                        seed=len(out) + 1 if seed is None else seed))
    # the matrix: typesize x size x filter (clevel / blocksize / codec vary along it so that the file stays small)
    sizes = [1, 15, 100, 4096, 70000, 300001]
    for ti, ts in enumerate([1, 2, 3, 4, 7, 8, 16, 17, 32, 255]):
        for si, size in enumerate(sizes):
            for filt in (0, 1, 2):
                k = ti + si + filt
                add(["f32", "text", "i16", "f64"][k % 4], size, ts, filt, clevel=[1, 5, 9][k % 3], cname=["lz4", "lz4hc"][k % 2],
                    blocksize=[0, 4096, 65536][(k // 2) % 3] if size > 4096 else 0)
    for split in (1, 2, 3, 4):                                          # always, never, auto, forward-compatible
        for ts in (4, 8):
            add("f32", 200000, ts, 1, split=split)
            add("f64", 40000, ts, 2, split=split, blocksize=4096)
    for bs in (4096, 65536, 1 << 20):
        for d in (-1, 0, 1):                                            # around block boundaries
            add("f32", 2 * bs + d if bs < (1 << 20) else bs + d, 4, 1, blocksize=bs)
            add("i16", 3 * bs + d if bs < (1 << 20) else bs + d, 2, 2, blocksize=bs)
    for ts, filt in ((1, 0), (4, 1), (8, 2)):
        add("rand", 20000, ts, filt)                                    # stored streams
        add("zeros", 150000, ts, filt)
        add("rand", 100, ts, filt, clevel=0)                            # memcpyed
    add("f32", 32768, 4, 1, blocksize=32768)                            # streams of 8 KiB   (<= 16 KiB)
    add("f32", 131072, 4, 1, blocksize=131072, seed=901)                # 32 KiB
    add("f32", 262144, 4, 1, blocksize=262144, seed=902)                # 64 KiB
    add("f32", 1 << 20, 4, 1, clevel=5, seed=903)                       # libblosc's default: 128 KiB streams
    add("text", 600000, 1, 0, blocksize=1 << 20, seed=904)              # one stream above 256 KiB
    add("text", 20000, 4, 1, cname="blosclz", seed=905)                 # refused formats
    add("text", 20000, 4, 1, cname="zstd", seed=906)
    add("text", 20000, 4, 1, cname="zlib", seed=907)
    return out


def mutations(valid):
    """seeded, structural: (name, base chunk's name, mutation) — blosc_model.mutate applies it, so that the file holds no second copy"""
    import numpy as np
    rng = np.random.default_rng(20260)
    out = []
    for (name, _index), chunk in valid:
        h, streams = M.parse(chunk)
        nb = h["nblocks"]
        cuts = sorted({0, 8, 15, 16, 17, 16 + 2 * nb, 16 + 4 * nb, 16 + 4 * nb + 2, len(chunk) // 2, len(chunk) - 1})
        for c in cuts:
            if c < len(chunk):
                out.append(("%s/cut%d" % (name, c), name, ["cut", c]))

        def put(off, fmt, val, tag):
            out.append(("%s/%s" % (name, tag), name, ["put", off, fmt, val]))
        put(12, "<I", h["cbytes"] + 1, "cbytes+1"); put(12, "<I", h["cbytes"] - 1, "cbytes-1"); put(12, "<I", 8, "cbytes8")
        put(4, "<I", h["nbytes"] + 1, "nbytes+1"); put(4, "<I", max(h["nbytes"] // 2, 1), "nbytes/2"); put(4, "<I", 0xFFFFFFF0, "nbytes-huge")
        put(4, "<I", 0, "nbytes0")
        put(8, "<I", 0, "blocksize0"); put(8, "<I", h["nbytes"] + 1, "blocksize>nbytes"); put(8, "<I", max(h["blocksize"] // 2, 1), "blocksize/2")
        put(8, "<I", 1, "blocksize1")
        put(0, "<B", 1, "version1"); put(0, "<B", 3, "version3"); put(1, "<B", 2, "versionlz2")
        put(2, "<B", h["flags"] | 5, "both-shuffles"); put(2, "<B", h["flags"] | 8, "reserved-flag"); put(2, "<B", h["flags"] ^ 16, "split-flipped")
        put(2, "<B", h["flags"] | 2, "memcpyed-set"); put(2, "<B", (h["flags"] & 31) | (4 << 5), "format-zstd")
        put(3, "<B", 0, "typesize0"); put(3, "<B", (h["typesize"] % 255) + 1, "typesize+1")
        if nb:
            put(16, "<I", 15, "bstart-in-header"); put(16, "<I", 16 + 4 * nb - 1, "bstart-in-table"); put(16, "<I", len(chunk), "bstart-end")
            put(16, "<I", len(chunk) - 3, "bstart-near-end"); put(16, "<I", 0xFFFFFFFF, "bstart-huge")
            if nb > 1:
                out.append((name + "/bstarts-swapped", name, ["swap", 16, 20, 4]))
                put(20, "<I", struct.unpack_from("<I", chunk, 16)[0], "bstarts-equal")
        if streams:
            s = streams[int(rng.integers(0, len(streams)))]
            put(s[0] - 4, "<i", -1, "word-negative"); put(s[0] - 4, "<i", 0, "word-zero"); put(s[0] - 4, "<i", 0x7FFFFFFF, "word-huge")
            put(s[0] - 4, "<i", len(chunk), "word-past-end"); put(s[0] - 4, "<i", s[1] + 1, "word+1")
            comp = [t for t in streams if not t[5] and t[1] >= 4]
            if comp:
                t = comp[int(rng.integers(0, len(comp)))]
                put(t[0], "<I", 0xFFFFFFFF, "lz4-damaged")
    return out


MUTATED = ["t4_s70000_f1", "t8_s4096_f2", "t17_s70000_f1", "t1_s100_f0", "t2_s300001_f2", "rand_t4", "t255_s70000_f0"]


def build(L):
    valid, by_tag, blob = [], {}, bytearray()
    for i, r in enumerate(recipes()):
        raw = M.make_input(r["kind"], r["size"], r["seed"])
        chunk = mint(L, raw, r)
        e = dict(recipe=r, nbytes=len(raw), sha256=hashlib.sha256(raw).hexdigest(), at=len(blob), len=len(chunk),
                 supported=r["cname"] in ("lz4", "lz4hc") or bool(chunk[2] & 2))
        valid.append(e)
        blob += chunk
        tag = ("rand_t%d" % r["typesize"]) if r["kind"] == "rand" and r["size"] == 20000 else "t%d_s%d_f%d" % (r["typesize"], r["size"], r["filter"])
        by_tag.setdefault(tag, ((tag, i), chunk))
    bad = []
    chunks = {tag: (i, c) for (tag, i), c in (by_tag[t] for t in MUTATED)}
    for name, tag, mut in mutations([by_tag[t] for t in MUTATED]):
        base, c = chunks[tag]
        b = M.mutate(c, mut)
        cls, out = M.verdict(b)
        e = dict(name=name, base=base, mutation=mut, verdict=cls)                   # base: index of the valid chunk it was made from
        if cls == "ok":
            e.update(sha256=hashlib.sha256(out).hexdigest(), nbytes=len(out))
        if len(b) >= 16:
            e["validate"] = validate(L, b)                                          # blosc_cbuffer_validate's answer, for information
        bad.append(e)
    return dict(valid=valid, malformed=bad), bytes(blob)


if __name__ == "__main__":
    L = load_libblosc()
    if L is None:
        sys.exit("libblosc.so.1 not found")
    import oracle
    oracle.build()
    doc, blob = build(L)
    path = os.path.join(HERE, "golden_blosc.json")
    line = lambda e: json.dumps(e, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"valid":[\n' + ",\n".join(line(e) for e in doc["valid"]) + '\n],"malformed":[\n' + ",\n".join(line(e) for e in doc["malformed"]) + "\n]}\n")
    with open(os.path.join(HERE, "golden_blosc.bin"), "wb") as f:
        f.write(blob)
    print(path, os.path.getsize(path), "bytes;", len(blob), "bytes of chunks;", len(doc["valid"]), "valid,", len(doc["malformed"]), "malformed")
