"""DEFLATE on the CPU: the kernel's own decoder (cramjam_amd/csrc/deflate_wave.hpp) compiled for the host with bounds-checked stand-ins
(tests/hostsim/sim_deflate_decode.cpp) against the fixtures zlib minted (tests/golden/golden_deflate.*), the hand-written streams and
the seeded mutations of tests/deflate_cases.py, and against Python's zlib live: at three input alignments, at capacities exact,
exact + 64, exact - 1 and 0, and in size mode.  Plus the fixtures' own coverage, the argument checks that need no device and the
lane-parallel checksums against zlib's.  No GPU."""
import ctypes as C
import zlib

import pytest

import deflate_cases as D


def test_fixtures_cover_the_matrix():
    vs, ms, hs = D.valid(), D.mutations(), D.hand()
    assert {v["payload"] for v in vs} == set(D.payloads()) | {"flush300k"}
    for p in ("empty", "one", "text300", "text4k"):
        assert sum(1 for v in vs if v["payload"] == p) == 48                 # the full cross
    big = [v for v in vs if v["n"] >= 65536]
    assert {v["level"] for v in big} == set(D.LEVELS) and {v["strategy"] for v in big} == set(D.STRATEGY_NAME.values()) and {v["wrap"] for v in big} == set(D.WRAPS)
    assert all(D.sha(D.payloads()[v["payload"]]) == v["sha256"] for v in vs if v["payload"] != "flush300k")
    assert max(v["n"] for v in vs) == 300000
    ok = sum(1 for m in ms if m["result"] >= 0)
    assert len(ms) == 600 and ok >= 60 and len(ms) - ok >= 60 and len({m["base"] for m in ms}) == 6
    assert {h["result"] for h in hs} >= {D.CORRUPT, D.HEADER, D.CHECKSUM, D.EOF, D.TRAILING} and sum(1 for h in hs if h["result"] >= 0) >= 10
    assert len(D.DIVERGES_FROM_ZLIB) <= 0.02 * (len(vs) + len(ms) + len(hs))


def test_fixtures_are_what_zlib_says_today():
    """the recorded verdicts against the zlib that is loaded now (and the hand-written streams against their recorded list)"""
    for c in D.cases():
        r, out = D.verdict(c["wrap"], c["bytes"], c["cap"])
        assert r == c["result"] and (r < 0 or (len(out) == c["n"] and D.sha(out) == c["sha256"])), c["name"]


def _caps(c):
    if c["result"] >= 0:
        n = c["result"]
        return [n, n + 64, 0] + ([n - 1] if n > 0 else [])
    return [c["cap"], 64, 0]


def test_kernels_decoder_on_the_host_equals_zlib_everywhere():
    """every fixture, hand-written stream and mutation: at its own capacity the fixture's verdict and bytes; at capacities exact,
    exact + 64, exact - 1 and 0 (rejected streams: their capacity, 64 and 0) zlib's live verdict at that capacity; three alignments"""
    runs = 0
    for c in D.cases():
        if c["name"] in D.DIVERGES_FROM_ZLIB:
            continue
        s, wrap = c["bytes"], c["wrap"]
        big = len(s) > 20000
        for k, cap in enumerate([c["cap"]] + _caps(c)):
            want = (c["result"], None) if k == 0 else D.verdict(wrap, s, cap)
            for mis in ((runs % 4,) if big and k else (0, 1, 3)):
                r, out = D.sim_decode(wrap, s, cap, mis)
                assert r == want[0], (c["name"], cap, mis, r, want[0])
                if r >= 0:
                    assert D.sha(out) == c["sha256"] if k == 0 else out == want[1], (c["name"], cap, mis)
                runs += 1
    assert runs >= 3 * 4 * (len(D.valid()) + len(D.mutations())) // 2


def test_size_mode_equals_the_decoded_lengths_and_the_decoders_errors_but_the_checksums():
    seen = set()
    for c in D.cases():
        want = D.size_verdict(c["wrap"], c["bytes"])
        for mis in (0, 1, 3):
            assert D.sim_decode(c["wrap"], c["bytes"], 0, mis, size=True)[0] == want, (c["name"], mis, want)
        full = D.verdict(c["wrap"], c["bytes"], None)[0]
        assert want == full or full == D.CHECKSUM, c["name"]
        seen.add((full, want < 0))
    assert (D.CHECKSUM, False) in seen and (D.CHECKSUM, True) in seen          # a bad checksum alone is sized; what follows it is still an error


def test_fresh_mutations_against_live_zlib():
    """seeded flips that are not in the fixture file, each wrapper"""
    g = D._lcg(77)
    for v in (v for v in D.valid() if v["name"] in ("text4k_l6_default_raw", "text4k_l6_default_zlib", "text4k_l6_default_gzip", "text300_l9_rle_raw", "text4k_l1_fixed_gzip")):
        for k in range(150):
            s = D.flip(v["bytes"], next(g) % (8 * v["len"]))
            cap = v["n"] + (0, 300, -1)[k % 3]
            want = D.verdict(v["wrap"], s, cap)
            got = D.sim_decode(v["wrap"], s, cap, k % 4)
            assert got[0] == want[0] and (got[0] < 0 or got[1] == want[1]), (v["name"], k, got[0], want[0])


def test_checksums_of_the_lanes_equal_zlibs():
    """Adler-32 and CRC-32 as the 64 lanes compute them, at the lengths where a lane's share changes shape"""
    for n in (0, 1, 3, 4, 5, 255, 256, 257, 259, 260, 511, 512, 513, 1023, 5552, 5553, 65521, 70001):
        raw = D.random_bytes(n, n) if n != 5553 else b"\xff" * n
        for wrap in (D.ZLIB, D.GZIP):
            s = D.compress(raw, 0 if n % 2 else 6, zlib.Z_DEFAULT_STRATEGY, wrap)
            assert D.sim_decode(wrap, s, n, n % 4) == (n, raw), (n, wrap)
            k = len(s) - (4 if wrap == D.ZLIB else 8)                           # the first byte of the checksum
            assert D.sim_decode(wrap, s[:k] + bytes([s[k] ^ 0x40]) + s[k + 1:], n)[0] == D.CHECKSUM, (n, wrap)


def test_argument_refusals_that_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    dev = lambda wrap, op, flags, n=0: L.cj_deflate_batch_device(None, wrap, op, flags, n, None, None, None, None, None, None, None, None)
    host = lambda wrap, op, flags, n=0: L.cj_deflate_batch_host(None, wrap, op, flags, n, None, None, None, None, None)
    for call in (dev, host):
        for wrap in D.WRAPS:
            assert call(wrap, N.OP_DECOMPRESS, 0) == 0                                        # n == 0 succeeds
            assert call(wrap, N.OP_COMPRESS, 0) == D.BAD_ARG                                  # decode only
            assert call(wrap, 2, 0) == D.BAD_ARG
            for flags in (1, 2, N.FLAG_FORCE_WAVE_PER_CHUNK, 0x80000000):
                assert call(wrap, N.OP_DECOMPRESS, flags) == D.BAD_ARG, flags
            assert call(wrap, N.OP_DECOMPRESS, 0, 3) == D.BAD_ARG                             # a batch without its pointers
        assert call(3, N.OP_DECOMPRESS, 0) == D.BAD_ARG and call(-1, N.OP_DECOMPRESS, 0) == D.BAD_ARG
    for wrap, flags, n, want in ((0, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, D.BAD_ARG), (1, 1, 0, D.BAD_ARG), (1, 0, 2, D.BAD_ARG)):
        assert L.cj_deflate_batch_sizes_device(None, wrap, flags, n, None, None, None, None, None) == want
        assert L.cj_deflate_batch_sizes_host(None, wrap, flags, n, None, None, None) == want
    for code, word in ((-40, "invalid"), (-41, "incorrect header check"), (-42, "incorrect data check"), (-43, "incomplete or truncated"), (-44, "unused data")):
        assert word in N.strerror(code), code
    from cramjam_amd import batch
    with pytest.raises(ValueError):
        batch.deflate_sizes([b"\x03\x00"], wrapper="lzma")
    assert C.sizeof(C.c_int) == 4
