"""The Blosc chunk format on the CPU: the model (tests/blosc_model.py) against the fixtures that c-blosc minted, and the product's
chunk grammar (cramjam_amd/csrc/blosc_grammar.hpp, compiled for the host) against the model on every fixture.  No GPU."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import blosc_cases as K
import blosc_model as M

ROOT = K.ROOT


def test_model_decodes_every_valid_fixture():
    assert len(K.valid()) >= 200
    for v in K.valid():
        out = M.decode(v["bytes"])
        assert len(out) == v["nbytes"] and hashlib.sha256(out).hexdigest() == v["sha256"], v["name"]
        assert out == K.raw_of(v), v["name"]                       # the recipe regenerates the input
    for v in K.valid(supported=False):
        assert M.verdict(v["bytes"])[0] == M.UNSUPPORTED, v["name"]


def test_fixtures_cover_the_engine_classes_and_the_grammar():
    lens, flags = set(), set()
    for v in K.valid():
        h, streams = M.parse(v["bytes"])
        flags.add(h["flags"] & 0x17)
        for s in streams:
            if not s[5]:
                lens.add(0 if s[3] <= 16384 else 1 if s[3] <= 32768 else 2 if s[3] <= 65536 else 3 if s[3] <= 262144 else 4)
    assert lens == {0, 1, 2, 3, 4}
    assert {0x00, 0x01, 0x04, 0x10, 0x11, 0x14} <= flags
    assert any(s[5] for v in K.valid() for s in M.parse(v["bytes"])[1])         # stored streams
    assert any(M.parse(v["bytes"])[0]["flags"] & 2 for v in K.valid())          # memcpyed chunks


@pytest.mark.parametrize("typesize", [1, 2, 3, 4, 7, 8, 16, 17, 33, 255])
def test_model_filters_are_inverses(typesize):
    rng = np.random.default_rng(typesize)
    for n in (0, 8, 64, 1000):
        for tail in sorted({0, min(1, typesize - 1), typesize - 1}):
            blk = rng.integers(0, 256, n * typesize + tail, dtype=np.uint8).tobytes()
            assert M.unshuffle(M.shuffle(blk, typesize), typesize) == blk
            assert M.bitunshuffle(M.bitshuffle(blk, typesize), typesize) == blk
            assert len(M.shuffle(blk, typesize)) == len(blk)


def test_model_filters_match_stored_streams():
    """a stored stream holds the filtered bytes as c-blosc wrote them: the model's forward filters must give exactly those"""
    seen = 0
    for v in K.valid():
        h, streams = M.parse(v["bytes"])
        if not any(s[5] for s in streams):
            continue
        raw, bs = K.raw_of(v), h["blocksize"]
        for src, ln, dst, dlen, b, stored in streams:
            if stored:
                blk = raw[b * bs:(b + 1) * bs]
                filt = M.apply_filter(blk, h["typesize"], M.block_mode(h["flags"], h["typesize"], len(blk)), True)
                assert filt[dst - b * bs:dst - b * bs + dlen] == v["bytes"][src:src + ln], v["name"]
                seen += 1
    assert seen >= 3


def test_malformed_fixtures_have_the_models_verdict():
    kinds = set()
    for m in K.malformed():
        cls, out = M.verdict(m["bytes"])
        assert cls == m["verdict"], m["name"]
        if cls == "ok":
            assert hashlib.sha256(out).hexdigest() == m["sha256"] and len(out) == m["nbytes"], m["name"]
        kinds.add(cls)
    assert {M.HEADER, M.UNSUPPORTED, M.CORRUPT} <= kinds


def test_grammar_header_agrees_with_the_model_on_every_fixture():
    L = K.grammar_sim()
    for e in K.doc()["valid"] + K.malformed():
        code, hdr, rows = K.sim_walk(L, e["bytes"])
        try:
            h, streams = M.parse(e["bytes"])
        except M.Refused as r:
            assert code == M.CODE[r.cls], (e["name"], code, str(r))
            continue
        assert code == 0, (e["name"], code)
        assert hdr == (h["version"], h["versionlz"], h["flags"], h["typesize"], h["nbytes"], h["blocksize"], h["cbytes"], h["nblocks"]), e["name"]
        assert rows == [(s[0], s[1], s[2], s[3], s[4], int(s[5])) for s in streams], e["name"]


def test_grammar_reads_nothing_outside_the_chunk_under_sanitizers():
    so = os.path.join(ROOT, "tests", "hostsim", "libsim_blosc_grammar_asan.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", so,
                           os.path.join(ROOT, "tests", "hostsim", "sim_blosc_grammar.cpp")])
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sim_blosc_asan_child.py"), so], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "walked" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_bit_transposition_and_block_mode_match_the_model():
    L = K.grammar_sim()
    rng = np.random.default_rng(8)
    for _ in range(200):
        x = rng.integers(0, 256, 8, dtype=np.uint8)
        want = np.frombuffer(M.bitshuffle(x.tobytes(), 1), np.uint8)
        got = L.sim_blosc_tr8(int.from_bytes(x.tobytes(), "little"))
        assert got.to_bytes(8, "little") == want.tobytes()
        assert L.sim_blosc_tr8(got) == int.from_bytes(x.tobytes(), "little")
    for flags in (0, 1, 4):
        for ts in (1, 2, 7, 255):
            for nb in (0, 1, ts - 1, ts, 8 * ts, 8 * ts + 1, 9 * ts, 64 * ts + 3):
                assert L.sim_blosc_block_mode(flags, ts, nb) == M.block_mode(flags, ts, nb), (flags, ts, nb)


def test_writer_layout_keeps_every_stream_within_64k():
    L = K.grammar_sim()
    out = (C.c_uint * 3)()
    for ts in (1, 2, 3, 4, 8, 16, 17, 255):
        for nbytes in (1, 31, 32, 127, 2047, 2048, 65535, 65536, 65537, 100001, 262144, 262145, 1 << 20, (1 << 23) + 5):
            for want in (0, 1, 4096, 65536, 1 << 20):
                L.sim_blosc_layout(nbytes, ts, want, out)
                bs, nblk, split = out[0], out[1], out[2]
                assert 0 < bs <= nbytes and nblk == -(-nbytes // bs), (ts, nbytes, want)
                if split:
                    assert bs % ts == 0 and bs // ts <= 65536 and 1 < ts <= 16
                else:
                    assert bs <= 65536
                assert (nbytes % bs) <= 65536


def test_fixtures_are_what_the_minting_script_writes():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_blosc as G
    lib = G.load_libblosc()
    if lib is None:
        pytest.skip("libblosc.so.1 is not installed: the fixtures cannot be re-minted here")
    recipes = G.recipes()
    assert len(recipes) == len(K.doc()["valid"])
    for i, (r, v) in enumerate(zip(recipes, K.doc()["valid"])):
        assert r == v["recipe"]
        assert G.mint(lib, M.make_input(r["kind"], r["size"], r["seed"]), r) == v["bytes"], v["name"]
