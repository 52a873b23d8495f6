"""Zlib and Zstd streams in Blosc chunks on the CPU (CJ_BLOSC_FLAG_READ_ZLIB / _ZSTD): the model (tests/blosc_zcodec_model.py: Python's
zlib and libzstd under blosc_model's container walk) against the fixtures that c-blosc minted and against c-blosc's own decoder, the
kernels' own stream decoders compiled for the host over every non-stored stream of every fixture chunk, the chunk grammar compiled for
the host with a flags word, and the checks of the two flags that need no device.  No GPU."""
import ctypes as C
import os
import sys

import pytest

import blosc_model as M
import blosc_zcodec_model as Z

SIM_BOUNDS = -9999

# Where the model (and with it the kernels) and libblosc 1.21.0 part, by the fixture's name.  No valid fixture may be listed.
DIVERGES_FROM_LIBBLOSC = {
    "zlib_stream_plus_one_byte": "libblosc hands the stream to zlib's uncompress, which stops at the end of the zlib stream and leaves the byte behind it "
                                 "alone; here one Blosc stream is exactly one zlib stream, so a byte behind it is CJ_E_DEFLATE_TRAILING and the chunk "
                                 "CJ_E_CORRUPT (libblosc's ZSTD_decompress refuses the same byte behind a Zstandard frame itself)",
}


def _libzstd():
    import zstd_cases
    try:
        return zstd_cases.libzstd()
    except OSError as ex:
        pytest.skip("no libzstd on this machine: %s" % ex)


def _libblosc():
    sys.path.insert(0, os.path.join(Z.ROOT, "tests", "golden"))
    import make_golden_blosc_zcodecs as G
    L = G.G.load_libblosc()
    if L is None:
        pytest.skip("libblosc.so.1 is not installed")
    return G, L


def test_model_reproduces_every_valid_fixture_and_every_recorded_verdict():
    _libzstd()
    assert len(Z.valid()) >= 80
    for v in Z.valid():
        out = Z.decode(v["bytes"])
        assert len(out) == v["nbytes"] and Z.sha(out) == v["sha256"] and out == Z.raw_of(v), v["name"]
        want = {"zlib": Z.FORMAT_ZLIB, "zstd": Z.FORMAT_ZSTD}[v["recipe"]["cname"]]
        assert len(v["bytes"]) >= 16 and v["bytes"][2] >> 5 == want and v["bytes"][1] == 1, v["name"]
        assert v["name"] not in DIVERGES_FROM_LIBBLOSC
    kinds = set()
    for m in Z.malformed() + Z.hand():
        cls, out = Z.verdict(m["bytes"], m["cap"])
        assert cls == m["verdict"], m["name"]
        if cls == "ok":
            assert Z.sha(out) == m["sha256"] and len(out) == m["nbytes"], m["name"]
        kinds.add(cls)
    assert kinds == {"ok", M.CORRUPT, M.HEADER, M.UNSUPPORTED, M.TOO_SMALL}
    assert 280 <= len(Z.malformed()) <= 340 and len({m["base"] for m in Z.malformed()}) == 4
    assert [h["verdict"] for h in Z.hand()] == [M.CORRUPT, M.CORRUPT]
    # without its flag every chunk with a stream is refused as unsupported, with the other format's flag too
    for v in Z.valid():
        f = Z.fmt_of(v["bytes"])
        if f is not None:
            assert Z.verdict(v["bytes"], None, 0)[0] == M.UNSUPPORTED and Z.verdict(v["bytes"], None, Z.FLAGS & ~Z.FLAG_OF[f])[0] == M.UNSUPPORTED, v["name"]


def _zstd_blocks(frame):
    """number of blocks of a single Zstandard frame without a dictionary id"""
    fhd = frame[4]
    single, fcs_code = (fhd >> 5) & 1, fhd >> 6
    at = 5 + (0 if single else 1) + ((1 << fcs_code) if fcs_code else single)
    n = 0
    while True:
        bh = int.from_bytes(frame[at:at + 3], "little")
        n += 1
        at += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
        if bh & 1:
            return n


def test_fixtures_cover_the_cells():
    for fmt, cname in ((Z.FORMAT_ZLIB, "zlib"), (Z.FORMAT_ZSTD, "zstd")):
        vs = [v for v in Z.valid() if v["recipe"]["cname"] == cname]
        cells = {(v["recipe"]["typesize"], v["recipe"]["filter"]) for v in vs if v["recipe"]["size"] == 4096}
        assert cells == {(ts, f) for ts in (1, 2, 4, 8, 16, 7) for f in (0, 1, 2)}
        assert {(v["recipe"]["split"], v["recipe"]["clevel"]) for v in vs if v["recipe"]["size"] == 20000 and v["recipe"]["kind"] == "f32"} == \
            {(s, c) for s in (1, 2, 4) for c in (1, 5, 9)}
        by = {}
        for v in vs:
            r, b = v["recipe"], v["bytes"]
            if Z.fmt_of(b) is None:
                by.setdefault("memcpyed" if v["nbytes"] else "empty", v)
                continue
            h, streams = Z.parse(b)
            stored = sum(s[5] for s in streams)
            modes = {M.block_mode(h["flags"], h["typesize"], min(h["blocksize"], h["nbytes"] - at)) for at in range(0, h["nbytes"], h["blocksize"])}
            if r["size"] == 70000 and h["blocksize"] == 8192:
                assert len(streams) == 9 and h["nblocks"] == 9 and h["flags"] & 16
                by["nine_blocks"] = v
            if r["size"] == 70000 and h["blocksize"] == 65536 and not h["flags"] & 16:
                assert len(streams) == h["typesize"] + 1                       # one split block and the leftover block, one stream
                by["split_and_leftover"] = v
            if max(s[3] for s in streams) >= 300000:
                by["one_big_stream"] = v
                if fmt == Z.FORMAT_ZSTD:
                    s = max(streams, key=lambda s: s[3])
                    assert _zstd_blocks(b[s[0]:s[0] + s[1]]) == 3                # three blocks of 128 KiB at most: the literal slot is used again
            if 0 < stored < len(streams) and r["kind"] == "f32lo":
                assert not h["flags"] & 16 and h["flags"] & 1
                by["one_stored_among_compressed"] = v
            if stored == len(streams):
                by["all_stored"] = v
            if h["flags"] & 4 and modes == {0}:
                by["bitshuffle_odd_direct"] = v
            if h["flags"] & 4 and modes == {0, 2}:
                by["bitshuffle_odd_leftover"] = v
            if h["flags"] & 1 and h["typesize"] == 1:
                by["shuffle_typesize1_direct"] = v
            by.setdefault("split" if not h["flags"] & 16 else "unsplit", v)
        assert set(by) == {"memcpyed", "empty", "nine_blocks", "split_and_leftover", "one_big_stream", "one_stored_among_compressed", "all_stored",
                           "bitshuffle_odd_direct", "bitshuffle_odd_leftover", "shuffle_typesize1_direct", "split", "unsplit"}, (cname, sorted(by))
    # the default split mode leaves Zstd blocks unsplit and splits Zlib blocks
    for v in Z.valid():
        r = v["recipe"]
        if r["split"] == 4 and r["size"] == 20000 and r["kind"] == "f32":
            assert bool(v["bytes"][2] & 16) == (r["cname"] == "zstd"), v["name"]
    kinds = {m["name"].split("/")[1].rstrip("0123456789=+-") for m in Z.malformed()}
    assert kinds == {"byte", "word", "versionlz", "format-snappy", "reserved-bit", "capacity"}, kinds


def test_fixtures_are_what_the_minting_script_writes():
    G, lib = _libblosc()
    _libzstd()
    version = G.libblosc_version(lib)
    if version != "1.21.0":
        pytest.skip("libblosc %s is not the 1.21.0 that minted the fixtures" % version)
    recipes = G.recipes()
    assert len(recipes) == len(Z.valid())
    pairs = []
    for r, v in zip(recipes, Z.valid()):
        assert r == v["recipe"] and v["libblosc_version"] == version
        chunk = G.G.mint(lib, Z.make_input(r["kind"], r["size"], r["seed"]), r)
        assert chunk == v["bytes"], v["name"]
        pairs.append((r, chunk))
    assert [(n, b, m) for n, b, m in G.mutations(pairs)] == [(m["name"], m["base"], m["mutation"]) for m in Z.malformed()]
    assert [(n, b) for n, b in G.hand_chunks()] == [(h["name"], h["bytes"]) for h in Z.hand()]


def test_model_agrees_with_c_blosc_except_where_listed():
    G, lib = _libblosc()
    _libzstd()
    seen = set()
    for v in Z.valid():
        r, got = G.libblosc_decode(lib, v["bytes"], v["nbytes"])
        assert r == v["nbytes"] and Z.sha(got) == v["sha256"], v["name"]
    for m in Z.malformed() + Z.hand():
        cls, out = Z.verdict(m["bytes"], m["cap"])
        r, got = G.libblosc_decode(lib, m["bytes"], m["cap"])
        assert r == m["libblosc"], m["name"]                                    # what it said when the fixtures were minted
        if (cls == "ok") != (r > 0):
            seen.add(m["name"])
        elif cls == "ok":
            assert r == len(out) and got == out, m["name"]
    assert seen == set(DIVERGES_FROM_LIBBLOSC)
    assert len(DIVERGES_FROM_LIBBLOSC) == 1                                     # (recorded in DESIGN.md 5.10)


def test_recorded_libblosc_answers_diverge_only_where_listed():
    """the same comparison from the file alone, where libblosc does not load"""
    seen = {m["name"] for m in Z.malformed() + Z.hand() if (m["verdict"] == "ok") != (m["libblosc"] > 0)}
    assert seen == set(DIVERGES_FROM_LIBBLOSC)


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    from hostsim_build import build_sim
    d = tmp_path_factory.mktemp("sim_zcodecs")
    zs = C.CDLL(build_sim("sim_zstd_decode.cpp", str(d / "libsim_zstd_decode.so")))
    zs.sim_zstd_decode.restype = C.c_longlong
    zs.sim_zstd_decode.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    df = C.CDLL(build_sim("sim_deflate_decode.cpp", str(d / "libsim_deflate_decode.so")))
    df.sim_deflate_decode.restype = C.c_longlong
    df.sim_deflate_decode.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    g = C.CDLL(build_sim("sim_blosc_grammar_flags.cpp", str(d / "libsim_blosc_grammar_flags.so")))
    g.sim_blosc_walk_flags.restype = C.c_longlong
    g.sim_blosc_walk_flags.argtypes = [C.c_void_p, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p]
    g.sim_blosc_header_flags.restype = C.c_longlong
    g.sim_blosc_header_flags.argtypes = [C.c_void_p, C.c_ulonglong, C.c_uint]
    return zs, df, g


def _sim_stream(sims, fmt, s, cap, mis):
    """(result, output bytes) of the kernel's own decoder on the host: the stream `mis` bytes behind a 16-byte boundary, capacity
    exactly cap; the output block has 64 guard bytes that must stay as they were"""
    zs, df, _g = sims
    buf = (C.c_ubyte * (len(s) + 48))()
    at = C.addressof(buf) + (-C.addressof(buf)) % 16 + mis
    C.memmove(at, bytes(s), len(s))
    out = C.create_string_buffer(b"\xa5" * (cap + 64), cap + 64)
    r = zs.sim_zstd_decode(0, at, len(s), out, cap) if fmt == Z.FORMAT_ZSTD else df.sim_deflate_decode(1, 0, at, len(s), out, cap)
    assert out.raw[cap:] == b"\xa5" * 64
    return r, out.raw[:cap]


def test_kernels_stream_decoders_on_the_host_agree_with_the_model(sims):
    """zstd_wave.hpp and deflate_wave.hpp (wrapper 1: zlib), the functions the kernels run, compiled for the host with every access
    bounds-checked (a violation is SIM_BOUNDS): every non-stored stream of every valid, malformed and hand-made chunk, at input
    misalignments 0, 1 and 3 and a capacity of exactly dst_len, gives the model's length and bytes, or is refused where the model
    refuses.  (Only the model's answer is kept per distinct stream; the host build runs on every stream of every chunk.)"""
    _libzstd()
    streams = [("%s#%d" % (v["name"], k), fmt, s, cap) for v in Z.valid() + Z.malformed() + Z.hand() for k, (fmt, s, cap) in enumerate(Z.streams_of(v["bytes"]))]
    assert len(streams) > 2000 and {f for _n, f, _s, _c in streams} == {Z.FORMAT_ZLIB, Z.FORMAT_ZSTD}
    model = {}
    good = bad = 0
    for name, fmt, s, cap in streams:
        if (fmt, s, cap) not in model:
            try:
                model[(fmt, s, cap)] = Z.decode_stream(fmt, s, cap)
            except M.Refused:
                model[(fmt, s, cap)] = None
        want = model[(fmt, s, cap)]
        for mis in (0, 1, 3):
            r, out = _sim_stream(sims, fmt, s, cap, mis)
            assert r != SIM_BOUNDS, (name, mis)
            if want is None:
                assert r != cap, (name, mis, r)                  # whatever code: blosc_batch's verdict makes it CJ_E_CORRUPT
                bad += 1
            else:
                assert r == cap and out == want, (name, mis, r)
                good += 1
    assert good > 5000 and bad > 600 and len(model) > 450


def test_a_stored_streams_row_reads_and_writes_nothing(sims):
    """blosc_batch leaves the row of a stored stream in the Zlib / Zstd ranges with in_len 0 and out_cap 0: both decoders end in 0 or
    an error code, which the verdict does not look at, and touch nothing"""
    for fmt in (Z.FORMAT_ZLIB, Z.FORMAT_ZSTD):
        for mis in (0, 1, 3):
            r, _out = _sim_stream(sims, fmt, b"", 0, mis)
            assert r <= 0 and r != SIM_BOUNDS, (fmt, mis, r)


def _walk(g, chunk, flags):
    buf = (C.c_ubyte * max(len(chunk), 1)).from_buffer_copy(chunk if chunk else b"\0")
    hdr = (C.c_uint * 9)()
    cap = 1 << 12
    rows = (C.c_uint * (6 * cap))()
    n = C.c_ulonglong(0)
    code = g.sim_blosc_walk_flags(buf, len(chunk), flags, hdr, rows, cap, C.byref(n))
    hc = g.sim_blosc_header_flags(buf, len(chunk), flags)
    assert hc in (0, -30, -31) and (hc == 0 or (code == hc and n.value == 0))          # a header's refusal is the walk's, before any stream
    return code, tuple(hdr), [tuple(rows[6 * i:6 * i + 6]) for i in range(min(n.value, cap))]


def test_grammar_on_the_host_admits_the_formats_only_with_their_flags(sims):
    g = sims[2]
    for v in Z.valid():
        b, f = v["bytes"], Z.fmt_of(v["bytes"])
        for flags in (0, 2, 8, 16, 24, 26):
            code, hdr, rows = _walk(g, b, flags)
            if f is None or flags & Z.FLAG_OF[f]:
                h, streams = Z.parse(b, flags)
                assert code == 0 and rows == [(s[0], s[1], s[2], s[3], s[4], int(s[5])) for s in streams], (v["name"], flags)
                assert hdr[4] == v["nbytes"] and hdr[7] == h["nblocks"] and hdr[8] == (f if f is not None else 1), (v["name"], flags)
            else:
                assert code == -31 and rows == [] and hdr[4] == v["nbytes"], (v["name"], flags)
        if f is not None:
            for name, mut, want in (("versionlz2", ["put", 1, "<B", 2], -31), ("versionlz0", ["put", 1, "<B", 0], -31),
                                    ("snappy", ["put", 2, "<B", (b[2] & 31) | (2 << 5)], -31), ("format5", ["put", 2, "<B", (b[2] & 31) | (5 << 5)], -31),
                                    ("reserved", ["put", 2, "<B", b[2] | 8], -30)):
                for flags in (0, 24, 26):
                    assert _walk(g, M.mutate(b, mut), flags)[0] == want, (v["name"], name, flags)
    for m in Z.malformed() + Z.hand():
        code, _hdr, rows = _walk(g, m["bytes"], Z.FLAGS)
        try:
            _h, streams = Z.parse(m["bytes"])
            assert code == 0 and rows == [(s[0], s[1], s[2], s[3], s[4], int(s[5])) for s in streams], m["name"]
        except M.Refused as r:
            assert code == M.CODE[r.cls], m["name"]


def test_flag_checks_that_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = N.BloscParams(4, 1, 5, 1, 0)
    for flags, want in ((0, 0), (2, 0), (8, 0), (16, 0), (24, 0), (10, 0), (18, 0), (26, 0),
                        (4, -101), (12, -101), (1, -101), (9, -101), (32, -101), (0x100, -101), (0x80000000, -101)):
        assert L.cj_blosc_batch_device(None, 0, None, None, None, None, None, None, None, 0, None, flags, None) == want, flags
        assert L.cj_blosc_batch_host(None, 0, flags, 0, None, None, None, None, None, None) == want, flags
        assert L.cj_blosc_chunk_sizes_device(None, flags, 0, None, None, None, None, None) == want, flags
        assert L.cj_blosc_chunk_sizes_host(None, flags, 0, None, None, None) == want, flags
    # reading flags: with CJ_OP_COMPRESS any nonzero word is a bad argument (and 0 stays fine)
    for flags in (2, 8, 16, 24, 26, 1, 4):
        assert L.cj_blosc_batch_device(None, 1, None, None, None, None, None, None, None, 0, C.byref(p), flags, None) == -101, flags
        assert L.cj_blosc_batch_host(None, 1, flags, 0, None, None, None, None, None, C.byref(p)) == -101, flags
    assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(p)) == 0
    # Zlib and Zstd stay refused as write codecs
    for codec in (3, 4):
        pz = N.BloscParams(4, 1, 5, codec, 0)
        assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(pz)) == N.E_BLOSC_UNSUPPORTED
    assert (N.BLOSC_FLAG_READ_ZLIB, N.BLOSC_FLAG_READ_ZSTD) == (8, 16)
    assert [N.BLOSC.read_flags(*a) for a in ((), (True,), (False, True), (False, False, True), (True, True, True))] == [0, 2, 8, 16, 26]
    with pytest.raises(ValueError):
        N.ZSTD.read_flags(zstd=True)                        # (the keywords are about Blosc chunks, not about the plain Zstandard batches)
    # cj_blosc_chunk_info takes no flags and keeps reporting the default reading, the header filled
    from cramjam_amd import blosc2
    for fmt, kw in ((Z.FORMAT_ZSTD, dict(zstd=True)), (Z.FORMAT_ZLIB, dict(zlib=True))):
        v = next(x for x in Z.valid() if Z.fmt_of(x["bytes"]) == fmt)
        info = N.BloscInfo()
        buf = (C.c_ubyte * len(v["bytes"])).from_buffer_copy(v["bytes"])
        assert L.cj_blosc_chunk_info(buf, len(v["bytes"]), C.byref(info)) == N.E_BLOSC_UNSUPPORTED
        assert info.nbytes == v["nbytes"] and info.flags >> 5 == fmt and info.versionlz == 1 and info.version == 2
        assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"]), **kw) == (0, v["nbytes"])
        assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"])) == (N.E_BLOSC_UNSUPPORTED, v["nbytes"])
        assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"]), blosclz=True) == (N.E_BLOSC_UNSUPPORTED, v["nbytes"])
        other = dict(zlib=True) if fmt == Z.FORMAT_ZSTD else dict(zstd=True)
        assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"]), **other) == (N.E_BLOSC_UNSUPPORTED, v["nbytes"])
        # versionlz 2 stays refused with the flag
        bad = (C.c_ubyte * len(v["bytes"])).from_buffer_copy(M.mutate(v["bytes"], ["put", 1, "<B", 2]))
        assert blosc2._info_nbytes(C.addressof(bad), len(v["bytes"]), **kw)[0] == N.E_BLOSC_UNSUPPORTED
