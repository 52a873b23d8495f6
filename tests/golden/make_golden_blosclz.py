"""Mint tests/golden/golden_blosclz.json (one entry per line) and golden_blosclz.bin (the chunks' bytes, back to back) from c-blosc 1.x
with cname = "blosclz": valid chunks of seeded inputs (tests/blosc_model.make_input: the inputs are regenerated, not stored) and
malformed chunks made by seeded byte mutations INSIDE compressed streams of three valid ones.  The verdict of a malformed chunk is the
model's (tests/blosclz_model.py); what blosc_decompress_ctx returned for it is recorded beside it (`libblosc`: nbytes or a code <= 0),
and tests/test_blosclz_model.py checks the two against each other where libblosc loads.  Loader and minting calls are
make_golden_blosc.py's.  Runs only where libblosc loads; no test runs it, test_blosclz_model.py re-mints the valid chunks to pin this
script to the file."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import blosc_model as M  # noqa: E402
import blosclz_model as Z  # noqa: E402
import make_golden_blosc as G  # noqa: E402


def recipes():
    out = []

    def add(kind, size, typesize, filt, clevel=5, blocksize=0, split=4, seed=None):
        out.append(dict(kind=kind, size=size, typesize=typesize, filter=filt, clevel=clevel, cname="blosclz", blocksize=blocksize, split=split,
                        seed=len(out) + 1 if seed is None else seed))
    # typesize x filter cells at the three sizes (clevel / blocksize / the data kind vary along them)
    for ti, ts in enumerate([1, 2, 3, 4, 7, 8, 16, 17, 32, 255]):
        for si, size in enumerate([100, 4096, 70000]):
            for filt in (0, 1, 2):
                k = ti + si + filt
                add(["f32", "text", "i16", "f64"][k % 4], size, ts, filt, clevel=[1, 5, 9][k % 3], blocksize=[0, 4096, 65536][(k // 2) % 3] if size > 4096 else 0)
    for split in (1, 2):                                                # always split, never split
        for ts in (4, 8):
            add("f32", 40000, ts, 1, split=split)
            add("text", 40000, ts, 0, split=split, blocksize=8192)
    for ts, filt in ((1, 0), (4, 1)):
        add("zeros", 150000, ts, filt)                                  # extended lengths (libblosc closes these streams with literals too)
    add("rand", 20000, 4, 1)                                            # stored streams
    add("rand", 100, 4, 1, clevel=0)                                    # memcpyed
    add("text", 300001, 1, 0, blocksize=1 << 20, seed=904)              # far distances; libblosc cuts it into 262 144 + 37 857: the largest minted stream is
                                                                        # exactly 256 KiB, the one above it is hand-written (blosclz_model.hand_streams)
    return out


MUTATED = [(4, 4096, 1), (1, 70000, 0), (8, 70000, 2)]       # (typesize, size, filter) of the three base chunks
PER_BASE = 100


def mutations(valid):
    """[(name, base index, mutation)]: one byte inside a compressed stream of the base chunk set to a seeded value"""
    import numpy as np
    rng = np.random.default_rng(20261)
    out = []
    for ts, size, filt in MUTATED:
        base = next(i for i, (r, _c) in enumerate(valid) if (r["typesize"], r["size"], r["filter"]) == (ts, size, filt))
        chunk = valid[base][1]
        comp = [s for s in Z.parse(chunk)[1] if not s[5]]
        assert comp, (ts, size, filt)
        for k in range(PER_BASE):
            s = comp[int(rng.integers(0, len(comp)))]
            # the head of a stream (its first controls), anywhere in it, or its last bytes
            where = [int(rng.integers(0, min(s[1], 8))), int(rng.integers(0, s[1])), s[1] - 1 - int(rng.integers(0, min(s[1], 4)))][k % 3]
            off = s[0] + where
            val = int(rng.integers(0, 256))
            if val == chunk[off]:
                val ^= 0x20
            out.append(("t%d_s%d_f%d/byte%d=%d" % (ts, size, filt, off, val), base, ["put", off, "<B", val]))
    return out


def libblosc_decode(L, chunk, nbytes):
    """blosc_decompress_ctx into a buffer of the chunk's own nbytes: (return code, bytes)"""
    dst = C.create_string_buffer(max(nbytes, 1))
    r = L.blosc_decompress_ctx(chunk, dst, nbytes, 1)
    return r, dst.raw[:max(r, 0)]


def build(L):
    valid, blob, pairs = [], bytearray(), []
    for r in recipes():
        raw = M.make_input(r["kind"], r["size"], r["seed"])
        chunk = G.mint(L, raw, r)
        assert chunk[2] >> 5 == 0 and Z.decode(chunk) == raw, r
        valid.append(dict(recipe=r, nbytes=len(raw), sha256=hashlib.sha256(raw).hexdigest(), at=len(blob), len=len(chunk)))
        blob += chunk
        pairs.append((r, chunk))
    bad = []
    for name, base, mut in mutations(pairs):
        b = M.mutate(pairs[base][1], mut)
        cls, out = Z.verdict(b)
        e = dict(name=name, base=base, mutation=mut, verdict=cls)
        if cls == "ok":
            e.update(sha256=hashlib.sha256(out).hexdigest(), nbytes=len(out))
        e["libblosc"] = libblosc_decode(L, b, valid[base]["nbytes"])[0]
        bad.append(e)
    return dict(valid=valid, malformed=bad), bytes(blob)


if __name__ == "__main__":
    L = G.load_libblosc()
    if L is None:
        sys.exit("libblosc.so.1 not found")
    doc, blob = build(L)
    path = os.path.join(HERE, "golden_blosclz.json")
    line = lambda e: json.dumps(e, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"valid":[\n' + ",\n".join(line(e) for e in doc["valid"]) + '\n],"malformed":[\n' + ",\n".join(line(e) for e in doc["malformed"]) + "\n]}\n")
    with open(os.path.join(HERE, "golden_blosclz.bin"), "wb") as f:
        f.write(blob)
    print(path, os.path.getsize(path), "bytes;", len(blob), "bytes of chunks;", len(doc["valid"]), "valid,", len(doc["malformed"]), "malformed")
