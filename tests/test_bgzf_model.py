"""BGZF without a GPU: the model of tests/bgzf_model.py against Python's gzip on every case, family by family; the
host build of the walk (cramjam_amd/csrc/bgzf_grammar.hpp, unchanged, tests/hostsim/sim_bgzf_grammar.cpp) against the model's verdict
and member list on every case, through ctypes and as a stand-alone program under AddressSanitizer and UBSan with every stream flush
against the end of its allocation; the argument checks that need no device; the bound's arithmetic."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import pytest

import bgzf_model as M
from hostsim_build import SANITIZE, build_sim

# What gzip.decompress makes of each malformed family.  It rejects all but two.  Zero padding behind the last member it tolerates
# (a stated deviation of this library: the walk refuses every byte behind the last member).  And the `bc` family — BSIZE off by
# one, below the minimum or past the end, a BC subfield of four bytes, none at all, an SLEN past XLEN — is damage to the extra field
# alone, which an RFC 1952 reader skips by XLEN without reading it: gzip finds the members by decoding them and reads these
# streams whole.  A BGZF reader finds the members by BSIZE and cannot.
GZIP_ACCEPTS = {"zero_padding", "bc"}
FAMILIES = {"cut", "bc", "magic", "crc", "isize", "data", "zero_padding", "garbage"}


def _gzip(s):
    try:
        return gzip.decompress(s)
    except (OSError, EOFError, gzip.zlib.error):
        return None


def test_case_list_covers_what_it_promises():
    names = M.cases()
    fams = {f for f, _ in names.values()}
    assert fams == FAMILIES | {"ok", "ok_cut"}
    for nm in (0, 1, 2, 64, 65, 300):
        for level in (0, 1, 9):
            assert len(M.walk(names["ok_members%d_level%d" % (nm, level)][1])[1]) in (nm, nm + 1)      # (+ the marker)
    assert sum(1 for f, _ in names.values() if f == "cut") > 100


def test_valid_cases_equal_gzip():
    for k, (fam, s) in M.cases().items():
        if fam.startswith("ok"):
            r, out = M.want(k)
            assert r == len(out) and out == _gzip(s), k


def test_malformed_cases_against_gzip_family_by_family():
    seen = set()
    for k, (fam, s) in M.cases().items():
        if fam.startswith("ok"):
            continue
        r, out = M.want(k)
        assert r < 0 and out == b"", (k, r)
        g = _gzip(s)
        assert (g is not None) == (fam in GZIP_ACCEPTS), (k, fam, r)
        seen.add(fam)
    assert seen == FAMILIES


def test_verdicts_of_the_families():
    w = {k: M.want(k)[0] for k in M.cases()}
    assert {w[k] for k, (f, _) in M.cases().items() if f in ("cut", "zero_padding", "garbage")} == {M.EOF}
    assert {w[k] for k, (f, _) in M.cases().items() if f in ("crc", "isize")} == {M.CHECKSUM}
    assert {w[k] for k, (f, _) in M.cases().items() if f == "magic"} == {M.HEADER}
    assert w["bsize_below_minimum"] == w["bc_slen4"] == w["bc_missing"] == w["slen_past_xlen"] == M.HEADER and w["bsize_past_end"] == M.EOF
    assert M.CORRUPT in {w[k] for k, (f, _) in M.cases().items() if f == "data"}
    # the capacity comes before the members, behind the walk
    s = M.cases()["crc_bit_member1"][1]
    total = M.sizes(s)
    assert M.decode(s, total - 1)[0] == M.OUT_TOO_SMALL and M.decode(s, total)[0] == M.CHECKSUM
    assert M.decode(M.cases()["garbage_byte"][1], 0)[0] == M.EOF


def _rows(mem):
    return b"".join(struct.pack("<QQQ", *m) for m in mem)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(build_sim("sim_bgzf_grammar.cpp", str(tmp_path_factory.mktemp("bgzf") / "libsim_bgzf_grammar.so")))
    L.sim_bgzf_walk.restype = C.c_longlong
    L.sim_bgzf_walk.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    return L


def test_host_build_of_the_walk_gives_the_models_verdict_and_members(sim):
    for k, (_, s) in M.cases().items():
        code, mem = M.walk(s)
        rows = (C.c_ulonglong * (3 * len(mem) + 3))()
        n = C.c_ulonglong()
        assert sim.sim_bgzf_walk(s, len(s), rows, len(mem) + 1, C.byref(n)) == code, k
        assert n.value == len(mem) and bytes(rows)[:24 * len(mem)] == _rows(mem), k
        assert n.value <= len(s) // 26 + 1


def test_walk_stand_alone_under_sanitizers_on_every_case(tmp_path):
    """a program of its own (SIM_MAIN), run directly: every stream is a heap block of exactly its size, so a read behind n ends it"""
    assert SANITIZE
    exe = build_sim("sim_bgzf_grammar.cpp", str(tmp_path / "sim_bgzf_grammar_main"), main=True, sanitize=True)
    cases = M.cases()
    path = str(tmp_path / "bgzf_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, s in cases.values():
            code, mem = M.walk(s)
            f.write(struct.pack("<IIq", len(s), len(mem), code) + s + _rows(mem))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(cases) in r.stdout


def test_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = C.c_void_p(64)                # (never dereferenced: the checks come first)
    for op in (N.OP_DECOMPRESS, N.OP_COMPRESS):
        assert L.cj_bgzf_batch_device(None, 0, op, 0, 0, None, None, None, None, None, None, None, None) == 0
        assert L.cj_bgzf_batch_host(None, 0, op, 0, 0, None, None, None, None, None) == 0
        assert L.cj_bgzf_batch_device(None, 0, op, 1, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
        assert L.cj_bgzf_batch_device(None, 1, op, 0, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
        assert L.cj_bgzf_batch_host(None, 0, op, 4, 1, p, p, p, p, p) == M.BAD_ARG
        assert L.cj_bgzf_batch_host(None, 1, op, 0, 0, None, None, None, None, None) == M.BAD_ARG
    assert L.cj_bgzf_batch_device(None, 0, 2, 0, 1, p, p, p, p, p, p, p, None) == M.BAD_ARG
    assert L.cj_bgzf_batch_host(None, 0, 2, 0, 0, None, None, None, None, None) == M.BAD_ARG
    assert L.cj_bgzf_sizes_device(None, 0, 0, 0, None, None, None, None, None) == 0
    assert L.cj_bgzf_sizes_host(None, 0, 0, 0, None, None, None) == 0
    assert L.cj_bgzf_sizes_device(None, 0, 1, 1, p, p, p, p, None) == M.BAD_ARG
    assert L.cj_bgzf_sizes_device(None, 1, 0, 1, p, p, p, p, None) == M.BAD_ARG
    assert L.cj_bgzf_sizes_host(None, 0, 8, 0, None, None, None) == M.BAD_ARG
    assert L.cj_bgzf_batch_device(None, 0, N.OP_DECOMPRESS, 0, 1, p, p, p, None, p, p, p, None) == M.BAD_ARG      # a null row pointer
    # the DEFLATE entries keep refusing what they refused: BGZF has entry points of its own
    assert L.cj_deflate_batch_device(None, 3, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None, None, None, None) == M.BAD_ARG


def test_bound_arithmetic():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    L = N.lib()
    want = {0: 28, 1: 1 + 31 + 28, 65279: 65279 + 31 + 28, 65280: 65311 + 28, 65281: 65311 + 32 + 28, 130560: 2 * 65311 + 28,
            0x7E000000: (0x7E000000 // 65280) * 65311 + (0x7E000000 % 65280 + 31) + 28, 0x7E000001: 0}
    for n, b in want.items():
        assert L.cj_bgzf_compress_bound(n) == b == M.compress_bound(n) == batch.bgzf_compress_bound(n), n
    # a member's bound is the gzip stream's with the 18-byte header for the 10-byte one; the largest fits BSIZE
    for p in (1, 2, 1000, 65279, 65280):
        assert L.cj_bgzf_compress_bound(p) == L.cj_deflate_compress_bound(p, N.DEFLATE_GZIP) + 8 + 28
    assert L.cj_deflate_compress_bound(65280, N.DEFLATE_GZIP) + 8 == 65311 <= 65536
