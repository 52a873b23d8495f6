"""The Zstandard decoder of the kernel (cramjam_amd/csrc/zstd_wave.hpp) compiled for the host (tests/hostsim/sim_zstd_decode.cpp)
against libzstd: the recorded fixtures are what the loaded libzstd says today; the decoder equals them on every fixture, hand-written
stream and mutation at three input alignments and at capacities exact, + 64 (canary), - 1 and 0; the size query and its documented
blind spots; the coverage matrix; the XXH64 lanes; the argument checks; a sanitizer build as a stand-alone program."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import zstd_cases as Z
from conftest import ROOT
from hostsim_build import SimBuildError, build_sim

SIM_SRC = os.path.join(ROOT, "tests", "hostsim", "sim_zstd_decode.cpp")
SIM_BOUNDS = -9999


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simz") / "libsimz.so")
    S = C.CDLL(build_sim(SIM_SRC, so))
    S.sim_zstd_decode.restype = C.c_longlong
    S.sim_zstd_decode.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    S.sim_zstd_xxh64.restype = C.c_longlong
    S.sim_zstd_xxh64.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_ulonglong)]
    return S


def _decode(S, stream, cap, mis=0, size=False):
    src = C.create_string_buffer(mis + len(stream) + 1)
    src.raw = b"\x77" * mis + stream + b"\x77"
    out = C.create_string_buffer(b"\xa5" * (cap + 64), cap + 64)
    r = S.sim_zstd_decode(1 if size else 0, C.addressof(src) + mis, len(stream), None if size else out, cap)
    return r, out.raw


def test_fixtures_are_what_libzstd_says_today():
    cases = Z.load_cases()
    assert len(cases) > 600
    for c in cases:
        for cap, want in zip(Z.capacities(c.cap), c.verdicts):
            r, out = Z.zstd_verdict(c.stream, cap)
            assert r == want and (r < 0 or cap != c.cap or Z.sha(out) == c.sha), (c.name, cap, r, want)
    for name, (s, data) in Z.hand_streams().items():
        if data is not None:
            assert Z.zstd_verdict(s, len(data)) == (len(data), data), name


def test_coverage_matrix_and_divergence_cap():
    cases = Z.load_cases()
    cover = set()
    for c in cases:
        if c.accepted and not c.name.startswith("mut_"):
            assert c.tags == Z.classify(c.stream), c.name
            cover |= c.tags
    assert [m for m in Z.COVERAGE if m not in cover] == []
    muts = [c for c in cases if c.name.startswith("mut_")]
    assert len(muts) == 600 and sum(c.accepted for c in muts) >= 60 and sum(not c.accepted for c in muts) >= 60
    assert set(Z.DIVERGES_FROM_ZSTD) <= {c.name for c in cases} and len(Z.DIVERGES_FROM_ZSTD) <= 0.02 * len(cases)


@pytest.mark.parametrize("mis", [0, 1, 3])
def test_decoder_equals_libzstd_at_every_capacity(sim, mis):
    for c in Z.load_cases():
        if c.name in Z.DIVERGES_FROM_ZSTD:
            continue
        for cap, want in zip(Z.capacities(c.cap), c.verdicts):
            r, out = _decode(sim, c.stream, cap, mis)
            assert r != SIM_BOUNDS, (c.name, cap)
            assert r == want, (c.name, cap, r, want)
            assert out[cap:] == b"\xa5" * 64, (c.name, cap)                       # nothing at or behind the capacity
            if r >= 0:
                assert out[r:cap] == b"\xa5" * (cap - r), (c.name, cap)           # nothing between the result and the capacity
                assert cap != c.cap or Z.sha(out[:r]) == c.sha, (c.name, cap)


def test_divergences_are_what_the_list_says(sim):
    by = {c.name: c for c in Z.load_cases()}
    r, _ = _decode(sim, by["legacy_v07"].stream, 300)
    assert r == Z.E_HEADER and by["legacy_v07"].verdicts[0] != Z.E_HEADER


def test_size_query_and_what_it_does_not_report(sim):
    """the header's statement (zstd_cases.size_query_may_miss): equal to the decoder but for the checksum, for what lies inside the
    blocks of a frame with a content size, and — in a frame without one — for what only decoding Huffman / Treeless literals finds.
    Bad offsets, literal overruns and the sequences' other rules ARE reported in frames without a content size."""
    by = {c.name: c for c in Z.load_cases()}
    for name in ("hand_bad_offset", "hand_literal_overrun", "hand_repeat_first"):
        assert by[name].verdicts[1] == Z.E_CORRUPT and not Z.any_frame_has_content_size(by[name].stream)
        assert _decode(sim, by[name].stream, 0, size=True)[0] == Z.E_CORRUPT, name
    missed = reported = 0
    for c in Z.load_cases():
        if c.name in Z.DIVERGES_FROM_ZSTD:
            continue
        d = c.verdicts[1]                                      # the decoder with room to spare
        q, _ = _decode(sim, c.stream, 0, size=True)
        assert q >= 0 or q in (Z.E_HEADER, Z.E_CORRUPT, Z.E_SRC_SIZE, Z.E_DICT, Z.E_CHECKSUM, -5), (c.name, q)
        if d >= 0:
            assert q == d, (c.name, q, d)
        elif d == Z.E_OUT_TOO_SMALL:                           # a capacity's verdict: the query has none
            continue
        elif q != d:
            missed += 1
            assert Z.size_query_may_miss(c.stream, d), (c.name, q, d)
        elif d == Z.E_CORRUPT and c.name.startswith("mut_") and not Z.any_frame_has_content_size(c.stream):
            reported += 1
    assert missed > 0 and reported > 0                         # both sides of the statement are exercised by mutations too


def test_xxh64_lanes_match_the_scalar_one(sim):
    data = bytes((i * 131 + 7) & 255 for i in range(1000))
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 95, 96, 100, 1000):
        buf = C.create_string_buffer(data[:n], max(n, 1))
        h = C.c_ulonglong(0)
        assert sim.sim_zstd_xxh64(buf, n, C.byref(h)) != SIM_BOUNDS, n
        assert h.value == Z.xxh64(data[:n]), n
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999


def test_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = C.create_string_buffer(64)
    a = C.addressof(p)
    assert L.cj_zstd_batch_host(None, 1, N.OP_DECOMPRESS, 0, 1, a, a, a, a, a) == -101
    assert L.cj_zstd_batch_host(None, 0, N.OP_COMPRESS, 0, 1, a, a, a, a, a) == -101
    assert L.cj_zstd_batch_host(None, 0, N.OP_DECOMPRESS, 1, 1, a, a, a, a, a) == -101
    assert L.cj_zstd_batch_device(None, 0, N.OP_DECOMPRESS, 2, 1, a, a, a, a, a, a, a, None) == -101
    assert L.cj_zstd_batch_sizes_host(None, 5, 0, 1, a, a, a) == -101
    assert L.cj_zstd_batch_sizes_device(None, 0, 8, 1, a, a, a, a, None) == -101
    assert L.cj_zstd_batch_host(None, 0, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None) == 0
    assert L.cj_zstd_batch_sizes_host(None, 0, 0, 0, None, None, None) == 0
    assert L.cj_zstd_batch_device(None, 0, N.OP_DECOMPRESS, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert L.cj_zstd_batch_host(None, 0, N.OP_DECOMPRESS, 0, 1, a, a, None, a, a) == -101
    assert L.cj_zstd_batch_sizes_host(None, 0, 0, 1, a, a, None) == -101
    for code in (-50, -51, -52, -53, -54):
        assert N.strerror(code).startswith("zstd: ")
    assert (N.E_ZSTD_HEADER, N.E_ZSTD_CORRUPT, N.E_ZSTD_CHECKSUM, N.E_ZSTD_SRC_SIZE, N.E_ZSTD_DICT) == (-50, -51, -52, -53, -54)


def test_sanitizer_build_runs_every_case_as_a_program(tmp_path):
    exe, cases_file = str(tmp_path / "simz_asan"), str(tmp_path / "cases.bin")
    try:
        build_sim(SIM_SRC, exe, main=True, sanitize=True)
    except SimBuildError as e:
        if "asan" in e.stderr or "ubsan" in e.stderr or "sanitize" in e.stderr:
            pytest.skip("the compiler has no sanitizer runtime")
        raise
    recs = []
    for c in Z.load_cases():
        if c.name in Z.DIVERGES_FROM_ZSTD:
            continue
        for k, (cap, want) in enumerate(zip(Z.capacities(c.cap), c.verdicts)):
            exp = Z.zstd_verdict(c.stream, cap)[1] if want > 0 else b""
            recs.append(struct.pack("<4Iq", 0, len(c.stream), cap, k % 4, want) + c.stream + exp)
    with open(cases_file, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, cases_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 bad" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
