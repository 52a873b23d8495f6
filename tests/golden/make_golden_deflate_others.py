"""Mint tests/golden/golden_deflate_others.json + golden_deflate_others.bin from two encoders that are not zlib: libdeflate (levels 1,
6, 9 and 12) and zopfli (default options but 3 iterations), loaded with ctypes from the machine that mints (their paths and the sha256
of each library file are recorded, as make_golden_deflate.py records zlib's version).  Payloads text300, text4k, corpus64k, zeros64k,
dist32768 and random64k of tests/deflate_cases.py and, for libdeflate, the first 200 000 bytes of the corpus' lcet10.txt; raw DEFLATE
throughout, zlib and gzip wrappers for text4k and corpus64k; thinned (THINNED below) so that each file stays under 1 MiB.  Plus 200
seeded single-bit flips and cuts of four of the streams.  Every entry carries zlib's verdict at capacity n and the sha256 of the output,
in the compact rows of golden_deflate.json (deflate_cases.others() / other_mutations() expand them).  Data only.

    python tests/golden/make_golden_deflate_others.py
"""
import bz2
import ctypes as C
import ctypes.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deflate_cases as D  # noqa: E402

ENCODERS = ("libdeflate1", "libdeflate6", "libdeflate9", "libdeflate12", "zopfli3")
PAYLOADS = ("text300", "text4k", "corpus64k", "zeros64k", "dist32768", "random64k")
WRAPPED = ("text4k", "corpus64k")                 # these also in a zlib and a gzip wrapper
# incompressible bytes are 64 KiB a stream and the long prefix about 70 KiB: the encoders listed meet them, every encoder meets the rest
THINNED = {"random64k": ("libdeflate1", "libdeflate12", "zopfli3"), "corpus200k": ("libdeflate1", "libdeflate6", "libdeflate9", "libdeflate12")}
MUTATION_BASES = ("text4k_libdeflate12_raw", "text4k_zopfli3_raw", "corpus64k_libdeflate6_zlib", "text300_libdeflate1_raw")
MUTATIONS, SLACK = 200, 1024


def find(name, soname):
    """the library's file: the path in DEFLATE_OTHERS_LIBDIR, a conda prefix or the running Python's, else wherever the loader looks"""
    dirs = [os.environ.get("DEFLATE_OTHERS_LIBDIR"), os.path.join(os.environ.get("CONDA_PREFIX", "/opt/conda"), "lib"), os.path.join(sys.prefix, "lib"),
            os.path.join(sys.base_prefix, "lib")]
    for d in dirs:
        if d and os.path.exists(os.path.join(d, soname)):
            return os.path.realpath(os.path.join(d, soname))
    p = ctypes.util.find_library(name)
    if p is None:
        raise OSError("no %s on this machine" % soname)
    return p


class ZopfliOptions(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("verbose", "verbose_more", "numiterations", "blocksplitting", "blocksplittinglast", "blocksplittingmax")]


def load():
    """(compress(encoder, data, wrap) -> bytes, {library: {path, sha256}}); OSError where either library does not load"""
    pd, pz = find("deflate", "libdeflate.so.0"), find("zopfli", "libzopfli.so.1")
    ld, lz = C.CDLL(pd), C.CDLL(pz)
    ld.libdeflate_alloc_compressor.restype = C.c_void_p
    ld.libdeflate_alloc_compressor.argtypes = [C.c_int]
    ld.libdeflate_free_compressor.argtypes = [C.c_void_p]
    for kind in ("deflate", "zlib", "gzip"):
        f = getattr(ld, "libdeflate_%s_compress" % kind)
        f.restype, f.argtypes = C.c_size_t, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        g = getattr(ld, "libdeflate_%s_compress_bound" % kind)
        g.restype, g.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t]
    lz.ZopfliInitOptions.argtypes = [C.POINTER(ZopfliOptions)]
    lz.ZopfliCompress.restype = None
    lz.ZopfliCompress.argtypes = [C.POINTER(ZopfliOptions), C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_size_t)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]

    def compress(encoder, data, wrap):
        if encoder.startswith("libdeflate"):
            kind = ("deflate", "zlib", "gzip")[wrap]
            c = ld.libdeflate_alloc_compressor(int(encoder[10:]))
            assert c
            out = C.create_string_buffer(getattr(ld, "libdeflate_%s_compress_bound" % kind)(c, len(data)))
            n = getattr(ld, "libdeflate_%s_compress" % kind)(c, data, len(data), out, len(out))
            ld.libdeflate_free_compressor(c)
            assert n
            return out.raw[:n]
        opt = ZopfliOptions()
        lz.ZopfliInitOptions(C.byref(opt))
        opt.numiterations = int(encoder[6:])
        p, n = C.POINTER(C.c_ubyte)(), C.c_size_t(0)
        lz.ZopfliCompress(C.byref(opt), (2, 1, 0)[wrap], data, len(data), C.byref(p), C.byref(n))      # ZOPFLI_FORMAT_DEFLATE / _ZLIB / _GZIP
        s = C.string_at(p, n.value)
        libc.free(p)
        return s

    with open(pd, "rb") as f, open(pz, "rb") as g:
        libs = {"libdeflate": {"path": pd, "sha256": D.sha(f.read())}, "zopfli": {"path": pz, "sha256": D.sha(g.read())}}
    return compress, libs


def matrix():
    """[(name, payload name, encoder, wrap)] in the order of the .bin"""
    rows = []
    for p in PAYLOADS + ("corpus200k",):
        for e in THINNED.get(p, ENCODERS):
            for w in D.WRAPS if p in WRAPPED else (D.RAW,):
                rows.append(("%s_%s_%s" % (p, e, D.WRAP_NAME[w]), p, e, w))
    return rows


def payload(name):
    if name == "corpus200k":
        with open(os.path.join(HERE, "corpus", "lcet10.txt.bz2"), "rb") as f:
            return bz2.decompress(f.read())[:200000]
    return D.payloads()[name]


def mint(compress):
    """(blob, stream rows [name, length, n, sha256], mutation rows [base index, bit, cut, result, n, sha256 or null])"""
    blob, rows, at = bytearray(), [], {}
    for name, p, e, w in matrix():
        raw = payload(p)
        s = compress(e, raw, w)
        r, out = D.verdict(w, s, len(raw))
        assert r == len(raw) and out == raw, name
        at[name] = (len(blob), len(s), w, len(raw))
        rows.append([name, len(s), len(raw), D.sha(raw)])
        blob.extend(s)
    names = [r[0] for r in rows]
    g = D._lcg(2025)
    muts = []
    for m in range(MUTATIONS):
        base = MUTATION_BASES[m % len(MUTATION_BASES)]
        off, ln, w, n = at[base]
        s = bytes(blob[off:off + ln])
        cut, bit = None, 0
        if m % 10 == 9:
            cut = next(g) % ln
            ms = s[:cut]
        else:
            # every other flip in the first 100 bytes: the block header and the code lengths
            bit = next(g) % (8 * (ln if m & 1 else min(ln, 100)))
            ms = D.flip(s, bit)
        r, out = D.verdict(w, ms, n + SLACK)
        muts.append([names.index(base), bit, cut, r, len(out), D.sha(out) if out else None])
    accepted = sum(1 for m in muts if m[3] >= 0)
    assert accepted >= 20 and len(muts) - accepted >= 20, accepted
    return bytes(blob), rows, muts


def main():
    compress, libs = load()
    blob, rows, muts = mint(compress)
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    lines = lambda rs, per: ",\n".join(",".join(dumps(r) for r in rs[k:k + per]) for k in range(0, len(rs), per))
    with open(os.path.join(HERE, "golden_deflate_others.bin"), "wb") as f:
        f.write(blob)
    with open(os.path.join(HERE, "golden_deflate_others.json"), "w") as f:
        import zlib
        f.write('{"zlib":%s,"libraries":%s,"mutation_slack":%d,\n"valid":[\n%s],\n"mutations":[\n%s]}\n'
                % (dumps(zlib.ZLIB_VERSION), dumps(libs), SLACK, lines(rows, 1), lines(muts, 4)))
    accepted = sum(1 for m in muts if m[3] >= 0)
    print("%d streams (%d bytes), %d mutations (%d accepted)" % (len(rows), len(blob), len(muts), accepted))
    assert len(blob) < (1 << 20) and os.path.getsize(os.path.join(HERE, "golden_deflate_others.json")) < (1 << 20)


if __name__ == "__main__":
    main()
