"""BloscLZ streams in Blosc chunks on the CPU: the model (tests/blosclz_model.py) against the fixtures that c-blosc minted and
against c-blosc's own decoder on the malformed ones, the hand-written edges of the stream grammar, and the checks of the new flag
that need no device.  No GPU."""
import ctypes as C
import hashlib
import os
import sys

import pytest

import blosc_model as M
import blosclz_model as Z

EXPECT_BAD = {"far_0000_one_short", "far_ffff_one_short", "match_one_over_cap", "literals_one_short", "lone_match_control",
              "lone_long_match_control", "match_without_its_code", "dist_op_plus_1", "short_of_cap", "split4_second_one_over"}


def _libblosc():
    sys.path.insert(0, os.path.join(Z.ROOT, "tests", "golden"))
    import make_golden_blosclz as G
    return G, G.G.load_libblosc()


def test_model_decodes_every_valid_fixture():
    assert len(Z.valid()) >= 100
    for v in Z.valid():
        out = Z.decode(v["bytes"])
        assert len(out) == v["nbytes"] and hashlib.sha256(out).hexdigest() == v["sha256"], v["name"]
        assert out == Z.raw_of(v), v["name"]
        assert v["bytes"][2] >> 5 == 0 and v["bytes"][1] == 1, v["name"]


def test_fixtures_cover_the_cases():
    cells, flags, far, ext, runs, ends_in_match, biggest = set(), set(), 0, 0, 0, 0, 0
    stored = memcpyed = 0
    for v in Z.valid():
        r = v["recipe"]
        cells.add((r["typesize"], r["filter"], r["size"]))
        h, streams = Z.parse(v["bytes"])
        memcpyed += bool(h["flags"] & 2)
        flags.add(h["flags"] & 0x17)
        for src, ln, _dst, dlen, _b, st in streams:
            stored += st
            if st:
                continue
            biggest = max(biggest, dlen)
            s = v["bytes"][src:src + ln]
            f, e, d1, last = _walk(s)
            far += f; ext += e; runs += d1; ends_in_match += last
    for ts in (1, 2, 3, 4, 7, 8, 16, 17, 32, 255):
        for filt in (0, 1, 2):
            for size in (100, 4096, 70000):
                assert (ts, filt, size) in cells
    assert {0x00, 0x01, 0x04, 0x10, 0x11} <= flags                  # split and unsplit blocks, the three filters
    assert far > 0 and ext > 0 and runs > 0 and stored > 0 and memcpyed > 0
    assert biggest == 262144                                        # libblosc cuts BloscLZ blocks at 256 KiB: the 300 001 byte chunk is 262 144 + 37 857
    assert max(cap for name, _s, cap in Z.hand_streams() if name not in EXPECT_BAD) > 262144      # the stream above 256 KiB is hand-written
    # c-blosc's own compressor closes every stream with literals (no minted stream ends in a match, the zeros chunks' included): the
    # streams that end in a match at the last byte of their capacity are the hand-written ones
    assert ends_in_match == 0
    assert sum(_walk(s)[3] for name, s, _cap in Z.hand_streams() if name.endswith("ends_at_cap")) == 3


def _walk(s):
    """(far distances, extended lengths, distance-1 matches, 1 if the stream ends in a match) of a VALID stream"""
    far = ext = d1 = 0
    ip, ctrl, n, last = 1, s[0] & 31, len(s), 0
    while True:
        if ctrl < 32:
            ip += ctrl + 1
            last = 0
        else:
            ofs = (ctrl & 31) << 8
            if ctrl >> 5 == 7:
                ext += 1
                while s[ip] == 255:
                    ip += 1
                ip += 1
            code = s[ip]; ip += 1
            if code == 255 and ofs == 31 << 8:
                far += 1; ip += 2
            elif ofs + code == 0:
                d1 += 1
            last = 1
        if ip >= n:
            return far, ext, d1, last
        ctrl = s[ip]; ip += 1


def test_hand_written_streams_have_the_expected_verdicts():
    seen = set()
    for e in Z.hand_chunks():
        assert (e["verdict"] == M.CORRUPT) == (e["name"] in EXPECT_BAD) and e["verdict"] in ("ok", M.CORRUPT), e["name"]
        seen.add(e["name"])
    assert EXPECT_BAD <= seen
    by = {n: (s, cap) for n, s, cap in Z.hand_streams()}
    R = Z._noise(80000, 77)
    s, cap = by["far_ffff_at_op"]
    assert Z.decode_stream(s, cap) == R[:73727] + R[:7] + b"xyz"                               # distance 73 727 reaches byte 0
    s, cap = by["dist_8191_plain"]
    assert Z.decode_stream(s, cap) == R[:8200] + R[9:14] + b"xyz"
    s, cap = by["code_255_not_far"]
    assert Z.decode_stream(s, cap) == R[:8000] + R[8000 - 7936:8000 - 7936 + 5] + b"xyz"       # an ordinary distance of 30 * 256 + 256
    s, cap = by["len_ext_ff_ff_00"]
    assert Z.decode_stream(s, cap) == R[:100] + (R[50:100] * 11)[:519] + b"xyz"
    s, cap = by["first_byte_e0_k"]
    assert Z.decode_stream(s, cap)[:10] == R[:10]
    s, cap = by["run_match_ends_at_cap"]
    assert Z.decode_stream(s, cap) == R[:3] + R[2:3] * 5000
    s, cap = by["above_256k_run_then_far_match"]
    big = R[:3] + R[2:3] * 265000 + R[3:60003]
    assert cap == 325056 and Z.decode_stream(s, cap) == big + big[len(big) - 60040:len(big) - 60040 + 50] + b"xyz"
    assert len(big) - 60040 < 265003 < len(big) - 60040 + 50 and len(big) > 262144          # the source straddles the run's end, the output lies above 256 KiB


def test_malformed_fixtures_have_the_models_verdict():
    bad = Z.malformed()
    assert 280 <= len(bad) <= 320 and len({m["base"] for m in bad}) == 3
    kinds = set()
    for m in bad:
        cls, out = Z.verdict(m["bytes"])
        assert cls == m["verdict"], m["name"]
        if cls == "ok":
            assert hashlib.sha256(out).hexdigest() == m["sha256"] and len(out) == m["nbytes"], m["name"]
        assert (cls == "ok") == (m["libblosc"] > 0), m["name"]                                 # what c-blosc said when they were minted
        kinds.add(cls)
    assert kinds == {"ok", M.CORRUPT}


def test_fixtures_are_what_the_minting_script_writes():
    G, lib = _libblosc()
    if lib is None:
        pytest.skip("libblosc.so.1 is not installed: the fixtures cannot be re-minted here")
    recipes = G.recipes()
    assert len(recipes) == len(Z.valid())
    pairs = []
    for r, v in zip(recipes, Z.valid()):
        assert r == v["recipe"]
        chunk = G.G.mint(lib, M.make_input(r["kind"], r["size"], r["seed"]), r)
        assert chunk == v["bytes"], v["name"]
        pairs.append((r, chunk))
    assert [(n, b, m) for n, b, m in G.mutations(pairs)] == [(m["name"], m["base"], m["mutation"]) for m in Z.malformed()]


# The one place where the rules of the model (and of the kernel) and libblosc 1.21.0 part: a stream whose last item is a match.  By
# the rules it ends there and is good when it filled its capacity; libblosc's decoder reads the next control byte without looking
# whether one is left and then fails on it, so it returns -1 for every such stream (its compressor never writes one: it closes a
# stream with literals).  Reading more than libblosc does is harmless, the bytes are determined; DESIGN.md 8 records it.
ENDS_IN_A_MATCH = {"match_ends_at_cap", "far_match_ends_at_cap", "run_match_ends_at_cap", "split4_end_in_matches", "split4_two_blocks"}


def test_model_agrees_with_c_blosc_on_malformed_and_hand_written_chunks():
    G, lib = _libblosc()
    if lib is None:
        pytest.skip("libblosc.so.1 is not installed")
    hand = [e for e in Z.hand_chunks() if e["name"] not in ENDS_IN_A_MATCH]
    assert len(hand) == len(Z.hand_chunks()) - len(ENDS_IN_A_MATCH)
    for m in Z.malformed() + hand:
        cls, out = Z.verdict(m["bytes"])
        nbytes = int.from_bytes(m["bytes"][4:8], "little")
        r, got = G.libblosc_decode(lib, m["bytes"], nbytes)
        assert (cls == "ok") == (r > 0), (m["name"], cls, r)
        if cls == "ok":
            assert r == len(out) and got == out, m["name"]


def test_flag_checks_that_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    p = N.BloscParams(4, 1, 5, 1, 0)
    for flags, want in ((0, 0), (2, 0), (1, -101), (3, -101), (4, -101), (0x100, -101), (0x80000000, -101)):
        assert L.cj_blosc_batch_device(None, 0, None, None, None, None, None, None, None, 0, None, flags, None) == want, flags
        assert L.cj_blosc_batch_host(None, 0, flags, 0, None, None, None, None, None, None) == want, flags
        assert L.cj_blosc_chunk_sizes_device(None, flags, 0, None, None, None, None, None) == want, flags
        assert L.cj_blosc_chunk_sizes_host(None, flags, 0, None, None, None) == want, flags
    # the flag is a reading flag: with CJ_OP_COMPRESS it is a bad argument (and 0 stays fine)
    assert L.cj_blosc_batch_device(None, 1, None, None, None, None, None, None, None, 0, C.byref(p), 2, None) == -101
    assert L.cj_blosc_batch_host(None, 1, 2, 0, None, None, None, None, None, C.byref(p)) == -101
    assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(p)) == 0
    # BloscLZ stays refused as a write codec, and cj_blosc_chunk_info keeps reporting the default reading
    pz = N.BloscParams(4, 1, 5, 0, 0)
    assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(pz)) == N.E_BLOSC_UNSUPPORTED
    v = next(x for x in Z.valid() if Z.is_blosclz(x["bytes"]))
    info = N.BloscInfo()
    buf = (C.c_ubyte * len(v["bytes"])).from_buffer_copy(v["bytes"])
    assert L.cj_blosc_chunk_info(buf, len(v["bytes"]), C.byref(info)) == N.E_BLOSC_UNSUPPORTED
    assert info.nbytes == v["nbytes"] and info.flags >> 5 == 0 and info.versionlz == 1
    from cramjam_amd import blosc2
    assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"]), True) == (0, v["nbytes"])
    assert blosc2._info_nbytes(C.addressof(buf), len(v["bytes"]), False) == (N.E_BLOSC_UNSUPPORTED, v["nbytes"])


def test_kernels_stream_decoder_on_the_host_agrees_with_the_model():
    """cramjam_amd/csrc/blosclz_wave.hpp, the function the kernel runs, compiled for the host (tests/hostsim/sim_blosclz_decode.cpp:
    every copy bounds-checked, a violation is SIM_BOUNDS = -9999): every compressed stream of the valid, malformed and hand-written chunks and every
    hand-written stream, at input alignments 0, 1 and 3, gives the model's verdict and bytes"""
    from hostsim_build import SIM_DIR, build_sim
    L = C.CDLL(build_sim("sim_blosclz_decode.cpp", os.path.join(SIM_DIR, "libsim_blosclz_decode.so")))
    L.sim_blosclz_decode.restype = C.c_longlong
    L.sim_blosclz_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    streams = [(name, s, cap) for name, s, cap in Z.hand_streams()]
    for v in Z.valid() + Z.malformed() + Z.hand_chunks():
        if Z.is_blosclz(v["bytes"]):
            streams += [(v["name"], v["bytes"][src:src + ln], dlen) for src, ln, _d, dlen, _b, stored in Z.parse(v["bytes"])[1] if not stored]
    assert len(streams) > 1500
    for name, s, cap in streams:
        try:
            want = Z.decode_stream(s, cap)
        except M.Refused:
            want = None
        for mis in (0, 1, 3):
            buf = (C.c_ubyte * (len(s) + 8))()
            assert C.addressof(buf) % 4 == 0
            C.memmove(C.addressof(buf) + mis, s, len(s))
            out = (C.c_ubyte * cap)()
            r = L.sim_blosclz_decode(C.addressof(buf) + mis, len(s), out, cap)
            assert r != -9999, (name, mis)                   # SIM_BOUNDS: a stand-in's check fired
            if want is None:
                assert r == -7, (name, mis, r)
            else:
                assert r == cap and bytes(out) == want, (name, mis, r)
