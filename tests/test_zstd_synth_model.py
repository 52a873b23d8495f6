"""The Zstandard decoder on streams libzstd never writes (tests/zstd_synth.py): the generator's every claim against libzstd alone; every
claimed feature found again by a reader that is not the writer (zstd_cases.deep_classify) and the coverage list complete; the host build
of the kernel's decoder (tests/hostsim/sim_zstd_decode.cpp) equal to the live libzstd on every case at capacities exact, + 64, - 1 and 0
and input misalignments 0..3, in size mode, on 3 000 seeded single-bit flips and on 20 flips of each point of the Huffman grid; no stand-in's bounds check ever fires; the recorded
verdicts (tests/golden/golden_zstd_synth.json) are what the generator and libzstd say today; a sanitizer build as a stand-alone program."""
import json
import os
import struct
import subprocess

import pytest

import zstd_cases as Z
import zstd_synth as S
from conftest import ROOT
from hostsim_build import SimBuildError, build_sim
from test_zstd_model import SIM_BOUNDS, SIM_SRC, _decode, sim  # noqa: F401  (sim: the host build, a module fixture)

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_zstd_synth.json")
_verdicts = {}


def cap_of(c):
    return c.cap


def verdicts(c):
    """libzstd's (result, bytes) at the four capacities, computed once"""
    if c.name not in _verdicts:
        _verdicts[c.name] = [Z.zstd_verdict(c.stream, cap) for cap in Z.capacities(cap_of(c))]
    return _verdicts[c.name]


def test_every_claim_of_the_generator_is_libzstd_s_verdict():
    cases = S.cases()
    assert len(cases) >= 800
    for c in cases:
        if c.expected is not None:
            assert Z.zstd_verdict(c.stream, len(c.expected)) == (len(c.expected), c.expected), c.name
        else:
            assert Z.zstd_verdict(c.stream, 1 << 19)[0] in (Z.E_HEADER, Z.E_CORRUPT, Z.E_CHECKSUM, Z.E_SRC_SIZE), c.name
            assert Z.zstd_verdict(c.stream, c.cap)[0] < 0, c.name
    for fam in S.FAMILIES:
        part = [c for c in cases if c.family == fam]
        assert part and 5 * sum(c.expected is None for c in part) >= len(part), fam         # refusals by construction: one in five at least


def test_every_claimed_feature_is_found_again_and_the_coverage_is_complete():
    cover = set()
    for c in S.cases():
        found = Z.deep_classify(c.stream)
        assert c.features <= found, (c.name, sorted(c.features - found))
        cover |= c.features
    assert [m for m in Z.DEEP_COVERAGE if m not in cover] == []
    assert {"w:%dsymbols" % k for k in (12, 13, 14)} <= cover                                # the weights' table on both sides of the limit


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_host_build_equals_libzstd_at_every_capacity(sim, mis):
    for c in S.cases():
        assert c.name not in Z.DIVERGES_FROM_ZSTD
        for cap, (want, data) in zip(Z.capacities(cap_of(c)), verdicts(c)):
            r, out = _decode(sim, c.stream, cap, mis)
            assert r != SIM_BOUNDS, (c.name, cap)
            assert r == want, (c.name, cap, r, want)
            assert out[cap:] == b"\xa5" * 64, (c.name, cap)
            if r >= 0:
                assert out[:r] == data and out[r:cap] == b"\xa5" * (cap - r), (c.name, cap)


def test_size_query_keeps_its_statement(sim):
    missed = 0
    for c in S.cases():
        d = verdicts(c)[1][0]                                  # the decoder with room to spare
        q, _ = _decode(sim, c.stream, 0, size=True)
        assert q != SIM_BOUNDS and (q >= 0 or q in (Z.E_HEADER, Z.E_CORRUPT, Z.E_SRC_SIZE, Z.E_DICT, Z.E_CHECKSUM, -5)), (c.name, q)
        if d >= 0:
            assert q == d, (c.name, q, d)
        elif d != Z.E_OUT_TOO_SMALL and q != d:
            missed += 1
            assert Z.size_query_may_miss(c.stream, d), (c.name, q, d)
    assert missed > 0


def test_three_thousand_single_bit_flips(sim):
    flips = S.flips(3000)
    assert {f[1] for f in flips} == set(S.FAMILIES)
    accepted = 0
    for name, _, s, base in flips:
        cap = cap_of(base)
        for room in (cap, cap + 64):
            want, data = Z.zstd_verdict(s, room)
            r, out = _decode(sim, s, room, len(s) & 3)
            assert r != SIM_BOUNDS and r == want and out[room:] == b"\xa5" * 64, (name, room, r, want)
            assert r < 0 or out[:r] == data, (name, room)
        accepted += want >= 0
    assert 100 < accepted < 2900                              # both verdicts are exercised


def test_grid_flips_follow_libzstd_s_choice_of_huffman_decoder(sim):
    """every point of the Huffman grid with its own 20 flips at the streams' ends and the jump table: where libzstd takes its
    double-symbol decoder (the rows of 20 000 and 131 072 literals) some of these are accepted by that decoder alone"""
    flips = S.grid_flips()
    assert len(flips) == 24 * 20
    verdict = {}
    for name, _, s, base in flips:
        for room in (base.cap, base.cap + 64):
            want, data = Z.zstd_verdict(s, room)
            r, out = _decode(sim, s, room, len(s) & 3)
            assert r != SIM_BOUNDS and r == want and out[room:] == b"\xa5" * 64, (name, room, r, want)
            assert r < 0 or out[:r] == data, (name, room)
        verdict.setdefault(base.name, []).append(want >= 0)
    assert len(verdict) == 24
    for n in (256, 1024, 4096, 20000, 131072):                 # every row has flips of both verdicts
        row = [x for name, v in verdict.items() if name.startswith("huf_grid_%d_" % n) for x in v]
        assert 15 <= sum(row) <= len(row) - 15, (n, sum(row))


def test_recorded_verdicts_are_what_generator_and_libzstd_say_today():
    assert os.path.getsize(GOLDEN) < (1 << 20)
    rec = json.load(open(GOLDEN))["cases"]
    now = S.recorded_entries()
    assert len(rec) == len(now)
    names = [c.name for c in S.cases()] + [f[0] for f in S.flips(600) + S.grid_flips()]
    for name, a, b in zip(names, rec, now):
        assert a == b, (name, a, b)


def test_sanitizer_build_runs_every_synthesized_case_as_a_program(tmp_path):
    exe, cases_file = str(tmp_path / "simz_asan"), str(tmp_path / "cases.bin")
    try:
        build_sim(SIM_SRC, exe, main=True, sanitize=True)
    except SimBuildError as e:
        if "asan" in e.stderr or "ubsan" in e.stderr or "sanitize" in e.stderr:
            pytest.skip("the compiler has no sanitizer runtime")
        raise
    recs = []
    for c in S.cases():
        for k, (cap, (want, data)) in enumerate(zip(Z.capacities(cap_of(c)), verdicts(c))):
            recs.append(struct.pack("<4Iq", 0, len(c.stream), cap, k % 4, want) + c.stream + (data if want > 0 else b""))
    with open(cases_file, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, cases_file], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "0 bad" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
