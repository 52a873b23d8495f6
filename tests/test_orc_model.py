"""ORC compression streams without a GPU: the fixture's condition; the model's walk (tests/orc_model.py) against the
chunk lists pyarrow's files gave; the host build of the walk (cramjam_amd/csrc/orc_grammar.hpp, unchanged, tests/hostsim/
sim_orc_grammar.cpp) against the model over every golden stream and every single-byte truncation of a dozen of them, through ctypes and
as a stand-alone program under AddressSanitizer and UBSan with every stream flush against the end of its allocation; the verdict
rules; the argument checks that need no device; the bound's arithmetic."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

import orc_model as M
from hostsim_build import SANITIZE, build_sim


def test_fixture_condition():
    """every codec and both block sizes hold a compressed and an original chunk; at 65 536 a stream of 16 chunks or more"""
    assert len(M.golden()) == 88
    for codec in M.KINDS:
        for bs in (65536, 262144):
            gs = M.golden_of(codec, bs)
            chunks = [c for g in gs for c in g["chunks"]]
            assert any(c[2] for c in chunks) and any(not c[2] for c in chunks), (codec, bs)
            assert all(c[3] <= bs for c in chunks)
            if bs == 65536:
                assert max(len(g["chunks"]) for g in gs) >= 16, codec
        # what the GPU cases lean on: a full block at either size, and a chunk of about 100 bytes
        assert M.golden_chunks(codec, 65536, min_decoded=65536) and M.golden_chunks(codec, 262144, min_decoded=262144)
        assert M.golden_chunks(codec, 65536, max_decoded=128)


def test_model_walk_gives_the_recorded_chunks_and_zlib_decodes_them():
    for g in M.golden():
        code, chunks = M.walk(g["stream"])
        assert code == 0 and chunks == [c[:3] for c in g["chunks"]], g["name"]
        assert M.frame([(o, g["stream"][off:off + n]) for off, n, o in chunks]) == g["stream"]
        assert sum(c[3] for c in g["chunks"]) == g["decoded_len"]
        if g["codec"] == "zlib":               # the one codec Python reads: the recorded digests are those of the decoded bytes
            parts = [g["stream"][off:off + n] if o else zlib.decompress(g["stream"][off:off + n], -15) for off, n, o in chunks]
            assert [M.digest(p) for p in parts] == [c[4] for c in g["chunks"]] and M.digest(b"".join(parts)) == g["sha256"], g["name"]
        else:                                  # ... for the others, those of the original chunks at least
            assert all(M.digest(g["stream"][c[0]:c[0] + c[1]]) == c[4] for c in g["chunks"] if c[2]), g["name"]


def walk_cases():
    """every golden stream, every single-byte truncation of a dozen of them (the short ones of every codec), and header edges"""
    cases = [g["stream"] for g in M.golden()]
    short = sorted((g for g in M.golden() if g["len"] <= 600), key=lambda g: (g["len"], g["name"]))[:12]
    assert len(short) == 12
    for g in short:
        cases += [g["stream"][:k] for k in range(g["len"])]
    cases += [b"", b"\x01", b"\x01\x00", b"\x01\x00\x00", b"\x01\x00\x00" * 3000, b"\x03\x00\x00", b"\x03\x00\x00x", b"\x02\x00\x00",
              b"\xff\xff\xff", b"\xff\xff\xff" + bytes(100), M.frame([(1, b"abc"), (0, b"")]) + b"\x08", M.frame([(1, bytes(70000))])]
    return cases


def test_model_walk_on_truncations():
    for s in walk_cases():
        code, chunks = M.walk(s)
        assert len(chunks) <= len(s) // 3
        end = chunks[-1][0] + chunks[-1][1] if chunks else 0
        assert (code == 0) == (end == len(s)) and code in (0, M.ORC_HEADER)
    assert M.walk(b"\x01\x00\x00" * 3000) == (0, [(3 * k + 3, 0, 1) for k in range(3000)])
    assert M.walk(b"\x03\x00\x00") == (M.ORC_HEADER, []) and M.walk(b"\x03\x00\x00x") == (0, [(3, 1, 1)])
    assert M.walk(b"ab") == (M.ORC_HEADER, [])


def _rows(chunks):
    return b"".join(struct.pack("<QQQ", *c) for c in chunks)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(build_sim("sim_orc_grammar.cpp", str(tmp_path_factory.mktemp("orc") / "libsim_orc_grammar.so")))
    L.sim_orc_walk.restype = C.c_longlong
    L.sim_orc_walk.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    L.sim_orc_bound.restype = C.c_ulonglong
    L.sim_orc_bound.argtypes = [C.c_ulonglong, C.c_ulonglong]
    return L


def test_host_build_of_the_walk_gives_the_models_verdict_and_chunks(sim):
    for s in walk_cases():
        code, chunks = M.walk(s)
        rows = (C.c_ulonglong * (3 * len(chunks) + 3))()
        n = C.c_ulonglong()
        assert sim.sim_orc_walk(s, len(s), rows, len(chunks) + 1, C.byref(n)) == code
        assert n.value == len(chunks) and bytes(rows)[:24 * len(chunks)] == _rows(chunks)
        assert n.value <= len(s) // 3


def test_walk_stand_alone_under_sanitizers_on_every_case(tmp_path):
    """a program of its own (SIM_MAIN), run directly: every stream is a heap block of exactly its size, so a read behind n ends it"""
    assert SANITIZE
    exe = build_sim("sim_orc_grammar.cpp", str(tmp_path / "sim_orc_grammar_main"), main=True, sanitize=True)
    cases = walk_cases()
    path = str(tmp_path / "orc_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for s in cases:
            code, chunks = M.walk(s)
            f.write(struct.pack("<IIq", len(s), len(chunks), code) + s + _rows(chunks))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(cases) in r.stdout


def test_verdict_rules():
    bs = 4096
    assert M.verdict(M.ORC_HEADER, [10], bs, 0) == M.ORC_HEADER                          # the walk first
    assert M.verdict(0, [], bs, 0) == 0 and M.verdict(0, [0, 0], bs, 0) == 0
    assert M.verdict(0, [bs, bs], bs) == 2 * bs and M.verdict(0, [bs, bs + 1], bs) == M.ORC_BLOCK
    assert M.verdict(0, [10, -40, bs + 1, -43], bs, 0) == -40 and M.verdict(0, [10, bs + 1, -40], bs, 0) == M.ORC_BLOCK     # stream order
    assert M.verdict(0, [10, 20], bs, 29) == M.OUT_TOO_SMALL and M.verdict(0, [10, 20], bs, 30) == 30
    assert M.verdict(0, [10, 20, 30], bs, 60, [None, -12, -7]) == -12 and M.verdict(0, [10, 20], bs, 30, [10, 20]) == 30
    assert M.verdict(0, [10, -40], bs, 5) == -40                                        # a chunk's size error before the capacity


def test_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = C.c_void_p(64)                # (never dereferenced: the checks come first)
    for kind in M.KINDS.values():
        for op in (N.OP_DECOMPRESS, N.OP_COMPRESS):
            assert L.cj_orc_batch_device(None, kind, op, 0, 65536, 0, None, None, None, None, None, None, None, None) == 0
            assert L.cj_orc_batch_host(None, kind, op, 0, 65536, 0, None, None, None, None, None) == 0
            assert L.cj_orc_batch_device(None, kind, op, 1, 65536, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
            assert L.cj_orc_batch_device(None, kind, op, 0, 0, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
            assert L.cj_orc_batch_host(None, kind, op, 0, (1 << 23) + 1, 1, p, p, p, p, p) == M.BAD_ARG
        assert L.cj_orc_batch_device(None, kind, 2, 0, 65536, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
        # block sizes: the format's 2^23 for reading, 262 144 for writing
        assert L.cj_orc_batch_host(None, kind, N.OP_DECOMPRESS, 0, 1 << 23, 0, None, None, None, None, None) == 0
        assert L.cj_orc_batch_host(None, kind, N.OP_COMPRESS, 0, 262144, 0, None, None, None, None, None) == 0
        assert L.cj_orc_batch_host(None, kind, N.OP_COMPRESS, 0, 262145, 0, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_orc_sizes_device(None, kind, 0, 1 << 23, 0, None, None, None, None, None) == 0
        assert L.cj_orc_sizes_host(None, kind, 0, 1, 0, None, None, None) == 0
        assert L.cj_orc_sizes_device(None, kind, 1, 65536, 1, p, p, p, p, None) == M.BAD_ARG
        assert L.cj_orc_sizes_host(None, kind, 0, 0, 0, None, None, None) == M.BAD_ARG
        assert L.cj_orc_batch_device(None, kind, N.OP_DECOMPRESS, 0, 65536, 1, p, p, p, None, p, p, p, None) == M.BAD_ARG      # a null row pointer
    for kind in (0, 3, 6, 7, -1):     # NONE, LZO, BROTLI, nothing
        assert L.cj_orc_batch_device(None, kind, N.OP_DECOMPRESS, 0, 65536, 0, None, None, None, None, None, None, None, None) == M.BAD_ARG
        assert L.cj_orc_sizes_host(None, kind, 0, 65536, 0, None, None, None) == M.BAD_ARG
    assert N.strerror(M.ORC_HEADER).startswith("orc:") and N.strerror(M.ORC_BLOCK).startswith("orc:")
    assert (N.E_ORC_HEADER, N.E_ORC_BLOCK) == (M.ORC_HEADER, M.ORC_BLOCK) == (-60, -61)


def test_codec_names():
    from cramjam_amd import batch
    for bad in ("lzo", "brotli", "none", "ZLIB", None, 1):
        with pytest.raises(ValueError):
            batch.orc_stream_sizes([b""], bad)
        with pytest.raises(ValueError):
            batch.orc_compress_streams([b""], bad)
        with pytest.raises(ValueError):
            batch.orc_decompress_streams([b""], bad, output_lens=[0])


def test_bound_arithmetic(sim):
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    L = N.lib()
    want = {(0, 65536): 0, (1, 65536): 4, (65535, 65536): 65538, (65536, 65536): 65539, (65537, 65536): 65543, (3 * 4096 + 5, 4096): 3 * 4096 + 5 + 12,
            (100, 1): 400, (262144, 262144): 262147, (0x7E000000, 262144): 0x7E000000 + 3 * (0x7E000000 // 262144), (0x7E000001, 262144): 0,
            (10, 0): 0, (10, 262145): 0}
    for (n, bs), b in want.items():
        assert L.cj_orc_compress_bound(n, bs) == b == M.compress_bound(n, bs) == batch.orc_compress_bound(n, bs), (n, bs)
        if b or n == 0:
            assert sim.sim_orc_bound(n, bs) == b
    assert batch.orc_compress_bound(1000) == 1003                  # (the default block size is ORC's: 262 144)
    # the bound is a stream of original chunks: frame() of the pieces has exactly that length
    for n, bs in ((0, 7), (1, 7), (6, 7), (7, 7), (8, 7), (26, 7)):
        assert len(M.frame([(1, bytes(min(bs, n - i))) for i in range(0, n, bs)])) == M.compress_bound(n, bs)
