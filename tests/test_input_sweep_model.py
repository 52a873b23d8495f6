"""The input sweep on the CPU (tests/input_cases.py): the builder is deterministic and its streams mean what was meant; the shares that
keep the sweep honest — how many cuts are accepted, which offsets are refused and why —, asserted from the oracle alone; and the host
builds of the kernels' own code (tests/hostsim: the lane walker, the LZ4 wavefront decoder plain, linked and with a dictionary, the Snappy
wavefront decoder) on every case that applies to them, with the oracle's result and bytes, the slot's surroundings untouched and no access outside the registered ranges — for the cuts of family A
that includes every read behind in_len.

The wavefront decoders are loaded into this process without a sanitizer: their accessors (tests/hostsim/sim_wave.hpp) check every access
and report SIM_BOUNDS; as stand-alone programs they run the same cases under -fsanitize=address,undefined.  The lane walker has no accessors of its own: it is built as a stand-alone program under
-fsanitize=address,undefined and run on a cases file in which every stream and every output slot is a heap block of exactly its size."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import capacity_cases as K
import input_cases as I
import lz4_dict_model as D
import oracle
from hostsim_build import SIM_DIR, build_sim

SIM_BOUNDS = -9999
WINDOWS = (65536, 32768, 16384)


def _key(cases):
    return [(c["stream"], c["bytes"], c.get("after"), c["cap"], c["result"], c["out"]) for c in cases]


def test_the_builder_is_deterministic():
    assert _key(I.a_lz4_cases.__wrapped__("a")) == _key(I.a_lz4_cases("a"))
    assert _key(I.a_snappy_cases.__wrapped__("b")) == _key(I.a_snappy_cases("b"))
    assert _key(I.b_lz4_cases.__wrapped__("b")) == _key(I.b_lz4_cases("b")) and _key(I.b_snappy_cases.__wrapped__("a")) == _key(I.b_snappy_cases("a"))
    assert I.grid_pairs.__wrapped__() == I.grid_pairs()
    for s in I.overlap_streams(16384)[::37]:
        k, v = (int(x) for x in s["name"].rsplit("/", 1)[1].split("."))
        t = I._overlap_stream(16384, k, len(I.overlap_streams(16384)) // I.VARIANTS, v, 0)
        assert (t["bytes"], t["elements"], t["raw"]) == (s["bytes"], s["elements"], s["raw"])


# ---- family C: the streams mean what was meant -------------------------------------------------------------------------------------------
def test_the_grid_is_the_issues():
    pairs = I.grid_pairs()
    assert len(pairs) == len(set(pairs)) == 1457 and len(I.PERIODS) == 47 and len(I.MATCHES) == 31
    assert sum(m < p for p, m in pairs) > 300 and sum(m > p for p, m in pairs) > 900          # the control and the overlaps


@pytest.mark.parametrize("win", WINDOWS)
def test_every_overlap_stream_decodes_to_renders_bytes_in_both_codecs(win):
    streams = I.overlap_streams(win)
    for s, cl, cs in zip(streams, I.c_lz4_cases(win), I.c_snappy_cases(win)):
        assert (cl["result"], cl["out"]) == (s["U"], s["raw"]), s["name"]
        assert (cs["result"], cs["out"]) == (s["U"], s["raw"]), s["name"]
        assert len(s["seqs"]) >= I.MIN_SEQS and len(s["seqs"][0][0]) >= 64 and len(s["tail"]) >= 12
        assert cl["cap"] <= win and len(cl["bytes"]) <= win - 32 and len(cs["bytes"]) <= win - 32
    assert {cl["cap"] - cl["U"] for cl in I.c_lz4_cases(win)} == {0, 64}


@pytest.mark.parametrize("win", WINDOWS)
def test_every_pair_meets_every_destination_alignment(win):
    """from render's positions: over the eight variants the match of every (period, length) pair starts at all eight residues modulo 8,
    with the pair's own offset and length in the stream"""
    seen = {}
    for s in I.overlap_streams(win):
        for j, p, m, i in s["grid"]:
            assert s["seqs"][j][1:] == (p, m) and s["pos"][j][2] - s["pos"][j][1] == m and s["pos"][j][1] >= p
            seen.setdefault((p, m), set()).add(s["pos"][j][1] % 8)
    assert len(seen) == 1457 and all(v == set(range(8)) for v in seen.values())


def test_the_dictionary_overlap_streams():
    d = D.dictionary(I.DICT_LEN)
    for s, c in zip(I.overlap_streams(65536, I.DICT_LEN), I.c_dict_cases()):
        assert (c["result"], c["out"]) == (s["U"], s["raw"]), s["name"]
        first = s["grid"][:I.C_DICT_MATCHES]
        assert len(first) == I.C_DICT_MATCHES and all(1 <= s["seqs"][j][1] - s["pos"][j][1] <= p for j, p, m, i in first)
        assert sum(s["seqs"][j][1] - s["pos"][j][1] < m for j, p, m, i in first) >= 20           # ... and run on into the output
        assert oracle.lz4_decompress_raw(s["bytes"], s["U"] + 64)[0] < 0                        # needs the dictionary
    assert len(d) == I.DICT_LEN


def test_the_big_overlap_streams():
    streams = I.big_overlap_streams()
    assert len(streams) == len(I.BIG_PERIODS) * len(I.BIG_MATCHES) * len(I.BIG_STARTS) == 96
    for s, cl, cs in zip(streams, I.c_big_cases("lz4"), I.c_big_cases("snappy")):
        assert (cl["result"], cl["out"]) == (s["U"], s["raw"]) and (cs["result"], cs["out"]) == (s["U"], s["raw"]), s["name"]
        at = {ms: (off, m) for (_, off, m), (_, ms, _) in zip(s["seqs"], s["pos"])}
        assert all(at.get(b - s["start"]) == (s["period"], s["match"]) for b in I.BOUNDS), s["name"]
        assert s["U"] > 98304 + 600


# ---- the shares ------------------------------------------------------------------------------------------------------------------------------
def test_family_a_lz4_shares():
    """at least 6 accepted lengths per (stream, capacity); both kinds of `after` carry the same expected values, and the oracle gives
    them whatever lies behind in_len"""
    L = oracle.lib()
    total = acc = 0
    for body in K.LZ4_BODIES:
        per = {}
        cs = I.a_lz4_cases(body)
        for own, ff in zip(cs[0::2], cs[1::2]):
            assert (own["kind"], ff["kind"]) == ("own", "ff") and ff["after"] == b"\xff" * I.AFTER
            assert (own["bytes"], own["cap"], own["result"], own["out"]) == (ff["bytes"], ff["cap"], ff["result"], ff["out"])
            for c in (own, ff):
                buf = np.frombuffer(c["bytes"] + c["after"] + b"\0", np.uint8)
                out = np.zeros(c["cap"] + 1, np.uint8)
                r = int(L.cjo_lz4_decompress_raw(buf.ctypes.data, len(c["bytes"]), out.ctypes.data, c["cap"]))
                assert (r if r >= 0 else K.CORRUPT) == c["result"] and (r < 0 or out[:r].tobytes() == c["out"]), (c["stream"], c["in_len"], c["kind"])
            per.setdefault((own["stream"], own["cap"]), []).append(own["result"] >= 0)
            total += 1; acc += own["result"] >= 0
        assert min(sum(v) for v in per.values()) >= 6, (body, sorted((sum(v), k) for k, v in per.items())[:3])
    assert 150 <= acc < total // 20 and total > 6000, (acc, total)


def test_family_a_snappy_shares():
    for body in K.SNAPPY_BODIES:
        cs = I.a_snappy_cases(body)
        true = [c for c in cs if c["declared"] == "true"]
        for c in true:
            assert (c["result"] >= 0) == (c["in_len"] == len(K.varint(c["U"])) + len(_elements(body, c["stream"]))), (c["stream"], c["in_len"])
            assert c["result"] < 0 or c["result"] == c["U"]
        assert len({c["result"] for c in true if c["result"] < 0}) >= 3
        pre = [c for c in cs if c["declared"] == "prefix"]
        assert all(c["result"] > 0 and c["result"] in (c["cap"], c["cap"] - 64) for c in pre)               # accepted, with what it declares
        for s in I._pick(K.snappy_streams(body)):                                                   # at least one per cut sequence: the cut on its first element
            at = {c["cut"] for c in pre if c["stream"] == s["name"]}
            tok = I._snappy_tokens(s, K.render(s["seqs"], s["tail"])[1], K.CUTS)
            assert all(len(K.varint(s["U"])) + t in at for t in tok), s["name"]
    for codec in ("lz4", "snappy"):
        cs = I.a_big_cases(codec)
        assert len(cs) > 400 and 4 <= sum(c["result"] >= 0 for c in cs) < len(cs) // 4


_els = {}


def _elements(body, name):
    if not _els.get(body):
        _els[body] = {s["name"]: s["elements"] for s in K.snappy_streams(body)}
    return _els[body][name]


def test_family_b_shares():
    """between a fifth and a third refused, and every refusal for the offset's own reason"""
    lz4 = [c for b in K.LZ4_BODIES[:2] for c in I.b_lz4_cases(b)]
    assert len(lz4) == 480
    for cs in (lz4, [c for b in K.LZ4_BODIES[:2] for c in I.b_dict_cases(b)], [c for b in K.SNAPPY_BODIES for c in I.b_snappy_cases(b)]):
        bad = [c for c in cs if c["result"] < 0]
        assert len(cs) / 5 <= len(bad) <= len(cs) / 3 + 1 or cs[0]["dict_len"], (len(bad), len(cs))
        for c in cs:
            assert (c["result"] < 0) == (c["off"] == 0 or c["off"] > c["ms"] + c["dict_len"]), (c["stream"], c["seq"], c["off"], c["ms"], c["result"])
            assert c["result"] < 0 or c["result"] == c["U"]
    d = [c for b in K.LZ4_BODIES[:2] for c in I.b_dict_cases(b)]
    assert {c["off"] - c["ms"] for c in d} >= {1, 2, I.DICT_LEN - 1, I.DICT_LEN, I.DICT_LEN + 1}
    assert sum(c["result"] < 0 for c in d) >= len(d) // 8
    for codec in ("lz4", "snappy"):
        cs = I.b_big_cases(codec)
        assert all(c["ms"] > 65536 for c in cs) and any(c["ms"] > 98304 for c in cs) and all((c["result"] < 0) == (c["off"] > c["ms"]) for c in cs)
    assert {c["form"] for b in K.SNAPPY_BODIES for c in I.b_snappy_cases(b)} == {1, 2, 3}


def test_the_preamble_cases():
    """the oracle follows snap: over-long forms of up to 10 bytes whose value fits 32 bits are accepted"""
    cs = {c["form"]: c for c in I.b_preamble_cases()}
    u = cs["minimal"]["U"]
    for n in range(2, 11):
        assert (cs["%d-bytes" % n]["result"], cs["%d-bytes" % n]["size"]) == (u, u) and len(cs["%d-bytes" % n]["bytes"]) == len(cs["elements-alone"]["bytes"]) + n
    assert cs["minimal"]["result"] == u and cs["minimal"]["out"] == cs["10-bytes"]["out"]
    for name in ("11-bytes", "2^32-1", "33-bits", "2^32", "lone-80", "lone-80-alone", "nothing"):
        assert cs[name]["result"] < 0, name
    assert cs["2^32-1"]["size"] == 0xFFFFFFFF and cs["33-bits"]["size"] < 0 and cs["2^32"]["size"] < 0 and cs["11-bytes"]["size"] < 0 and cs["nothing"]["size"] == 0


def test_the_size_query_cases():
    cs = I.size_cases()
    acc = [c for c in cs if c["result"] >= 0]
    assert len(acc) >= 100 and len(cs) - len(acc) >= 1000, (len(acc), len(cs))
    assert any(0 < c["result"] < c["U"] for c in acc)                        # a cut the size walk accepts short of the whole stream


# ---- the host builds of the kernels' own code -----------------------------------------------------------------------------------------------
def _lz4_small_cases():
    """every LZ4 case of A, B and C that a chunk-sized decoder takes (the big streams are the slab path's)"""
    out = [c for b in K.LZ4_BODIES for c in I.a_lz4_cases(b)] + [c for b in K.LZ4_BODIES[:2] for c in I.b_lz4_cases(b)]
    return out + [c for w in WINDOWS for c in I.c_lz4_cases(w)]


G = 64


def _held(call, cases, hist=b""):
    """every case through call(in, n, out, cap) at misalignment n % 4, the stream registered as [0, in_len) (a read of `after` is
    SIM_BOUNDS): the case's result and bytes, 64 bytes of 0xA5 on both sides and [result, cap) untouched (hist: bytes that lie directly
    in front of the output in place of the guard, and are unchanged afterwards); returns the number of runs"""
    front = np.frombuffer(hist, np.uint8) if hist else np.full(G, 0xA5, np.uint8)
    for n, c in enumerate(cases):
        mis = n % 4
        src = b"\0" * mis + c["bytes"] + c.get("after", b"")
        buf = C.create_string_buffer(src, len(src) + 1)
        out = np.full(len(front) + c["cap"] + G, 0xA5, np.uint8)
        out[:len(front)] = front
        r = call(C.addressof(buf) + mis, len(c["bytes"]), out.ctypes.data + len(front), c["cap"])
        tag = (c["stream"], c.get("in_len"), c.get("kind"), c.get("off"), c.get("form"), c["cap"], r, c["result"])
        assert r != SIM_BOUNDS, tag
        assert r == c["result"] and (r <= 0 or out[len(front):len(front) + r].tobytes() == c["out"]), tag
        keep = max(r, 0) if r >= 0 else c["cap"]
        assert (out[:len(front)] == front).all() and (out[len(front) + keep:] == 0xA5).all(), tag
    return len(cases)


def _dict_cases():
    return [c for b in K.LZ4_BODIES[:2] for c in I.b_dict_cases(b)] + I.c_dict_cases()


def test_lz4_wavefront_host_build_on_every_lz4_case():
    """lz4_wave.hpp over sim_wave.hpp's checked accessors: lz4_wave_decode<false>, the text of lz4_decode_kernel, with hist = 0 on A, B
    and C; lz4_wave_decode<true>, lz4_dict_decode_kernel's, on B's and C's dictionary cases"""
    from test_lz4_dict_model import sim_lib
    L = sim_lib()
    d = D.dictionary(I.DICT_LEN)
    dbuf = C.create_string_buffer(d, len(d))
    plain = _lz4_small_cases()
    runs = _held(lambda p, n, out, cap: L.sim_lz4_wave_decode(p, n, out, cap, 0), plain)
    runs += _held(lambda p, n, out, cap: L.sim_lz4_dict_decode(p, n, out, cap, C.addressof(dbuf), len(d)), _dict_cases())
    assert runs == len(plain) + len(_dict_cases()) and runs > 14000


def test_lz4_wavefront_host_build_in_the_linked_form():
    """lz4_frame_chain_kernel's call shape: lz4_wave_decode<false> with the dictionary's bytes directly in front of the output and
    hist = DICT_LEN gives every dictionary case its own result and bytes, and leaves the history as it was"""
    from test_lz4_dict_model import sim_lib
    L = sim_lib()
    d = D.dictionary(I.DICT_LEN)
    assert len(d) == I.DICT_LEN == 4096
    cases = _dict_cases()
    assert _held(lambda p, n, out, cap: L.sim_lz4_wave_decode(p, n, out, cap, len(d)), cases, hist=d) == len(cases) > 0


def snappy_sim_lib():
    L = C.CDLL(build_sim("sim_snappy_wave.cpp", os.path.join(SIM_DIR, "libsim_snappy_wave.so")))
    L.sim_snappy_wave_decode.restype = C.c_longlong
    L.sim_snappy_wave_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    return L


def _snappy_cases():
    """every Snappy case of A, B and C that a chunk-sized decoder takes, and the preamble's forms"""
    out = [c for b in K.SNAPPY_BODIES for c in I.a_snappy_cases(b)] + [c for b in K.SNAPPY_BODIES for c in I.b_snappy_cases(b)]
    return out + [c for w in WINDOWS for c in I.c_snappy_cases(w)] + I.b_preamble_cases()


def test_snappy_wavefront_host_build_on_every_snappy_case():
    """snappy_wave.hpp, the text of snappy_decode_kernel, over sim_wave.hpp's checked accessors: the cuts, the offset edges in every copy
    form, the overlap grid of the three windows and the preamble's forms, held as the GPU sweep holds the wave mode"""
    L = snappy_sim_lib()
    cases = _snappy_cases()
    assert _held(L.sim_snappy_wave_decode, cases) == len(cases) > 3000


def _ten_byte_preambles():
    """the declared length in ten bytes whose last one is above 1 (bits that a u64 does not have: snap's Header error), in front of the
    preamble cases' element stream; the oracle decides"""
    c = next(c for c in I.b_preamble_cases() if c["form"] == "elements-alone")
    head = bytes(((c["U"] >> (7 * i)) & 127) | 128 for i in range(9))
    out = [dict(c, form="10-bytes-last-%d" % last, bytes=head + bytes([last]) + c["bytes"]) for last in (2, 3, 0x7F)]
    for x in out:
        x["result"], x["out"] = oracle.snappy_decompress(x["bytes"], x["cap"])
        x["result"] = int(x["result"])
    return out


def test_snappy_wavefront_host_build_on_the_capacity_sweep_and_ten_byte_preambles():
    """two rules that the input sweep's cases do not reach: a copy that would pass the declared length, where the declared length is the
    capacity (tests/capacity_cases.py: a write behind it is SIM_BOUNDS), and the tenth preamble byte above 1"""
    L = snappy_sim_lib()
    ten = _ten_byte_preambles()
    assert all(c["result"] < 0 for c in ten) and len({c["result"] for c in ten}) == 1
    cases = [c for b in K.SNAPPY_BODIES for c in K.snappy_cases(b)] + ten
    assert _held(L.sim_snappy_wave_decode, cases) == len(cases)


def write_lane_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for n, c in enumerate(cases):
            f.write(struct.pack("<IIIq", len(c["bytes"]), c["cap"], n % 4, c["result"]))
            f.write(c["bytes"]); f.write(c["out"])


def test_lane_walker_stand_alone_under_sanitizers_on_every_lz4_case(tmp_path):
    """lz4_lane_walk.hpp as a program of its own (tests/hostsim/sim_lane_walk.cpp, SIM_MAIN) under AddressSanitizer and UBSan: streams
    and slots are heap blocks of exactly their size, so a read behind in_len or a write outside the slot ends the program"""
    from test_hostsim_lane_walk import _build
    _build()                                             # (writes the header's body next to the sim; its shared object is not used here)
    exe = build_sim("sim_lane_walk.cpp", os.path.join(SIM_DIR, "sim_lane_walk_input_sweep"), main=True, sanitize=True)
    cases = _lz4_small_cases()
    path = str(tmp_path / "lane_cases.bin")
    write_lane_cases(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(cases) in r.stdout


def _run_cases_file(tmp_path, source, recs):
    exe = build_sim(source, str(tmp_path / "sim_main"), main=True, sanitize=True)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "%d cases, 0 bad" % len(recs) in r.stdout


def test_lz4_wavefront_stand_alone_under_sanitizers(tmp_path):
    """tests/hostsim/sim_lz4_wave.cpp as a program of its own (SIM_MAIN) under AddressSanitizer and UBSan, every block a heap block of
    exactly its size: the plain entry on every LZ4 case, the linked entry (the dictionary as history in front of the output) and the
    dictionary entry on every dictionary case"""
    d = D.dictionary(I.DICT_LEN)
    rec = lambda n, c, dl, linked: struct.pack("<6Iq", len(c["bytes"]), c["cap"], dl, n % 4, 3, linked, c["result"]) + c["bytes"] + d[:dl] + c["out"]
    recs = [rec(n, c, 0, 1) for n, c in enumerate(_lz4_small_cases())]
    recs += [rec(n, c, len(d), linked) for linked in (1, 0) for n, c in enumerate(_dict_cases())]
    _run_cases_file(tmp_path, "sim_lz4_wave.cpp", recs)


def test_snappy_wavefront_stand_alone_under_sanitizers(tmp_path):
    """tests/hostsim/sim_snappy_wave.cpp likewise, on every Snappy case"""
    recs = [struct.pack("<3Iq", len(c["bytes"]), c["cap"], n % 4, c["result"]) + c["bytes"] + c["out"] for n, c in enumerate(_snappy_cases())]
    _run_cases_file(tmp_path, "sim_snappy_wave.cpp", recs)
