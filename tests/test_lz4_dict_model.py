"""LZ4 blocks against a shared dictionary on the CPU: the model (tests/lz4_dict_model.py) against the fixtures the system liblz4
minted and, where it loads, against LZ4_decompress_safe_usingDict itself; the kernel's own decoder (cramjam_amd/csrc/lz4_wave.hpp, kDict = true)
compiled for the host with bounds-checked copies; the encoder's model with the dictionary as its history; the argument checks that
need no device.  No GPU."""
import ctypes as C
import os

import pytest

import lz4_dict_model as D
from hostsim_build import SIM_DIR, build_sim

SIM_BOUNDS = -9999

_mem = {}


def model_verdict(c, dict_len):
    """(result, bytes) of the model for a fixture stream, computed once"""
    key = (c["name"], dict_len)
    if key not in _mem:
        _mem[key] = D.decode(c["bytes"], c["cap"], D.dictionary(dict_len))
    return _mem[key]


def test_fixtures_cover_the_cases():
    vs = D.valid()
    assert {(v["dict_len"], v["size"]) for v in vs} == {(dl, n) for dl in D.DICT_LENS for n in D.RECORD_SIZES}
    assert D.meta()["have_hc"] and {v["hc"] for v in vs} == {False, True}
    assert D.meta()["needs_dictionary"] >= len(vs) // 3
    ms = D.mutations()
    ok = sum(1 for m in ms if m["result"] >= 0)
    assert len(ms) >= 300 and ok >= 50 and len(ms) - ok >= 50
    assert all(m["result"] >= 0 or m["result"] == D.CORRUPT for m in ms)
    hs = D.hand()
    assert sum(h["accepted"] for h in hs) >= 20 and sum(not h["accepted"] for h in hs) >= 10
    assert max(h["cap"] for h in hs) > 65536
    for dl in D.DICT_LENS:
        assert len(D.cases(dl)) >= 22
    assert sum(len(D.cases(dl)) for dl in D.BATCH_DICT_LENS) == len(vs) + len(ms) + len(hs)


def test_model_reproduces_every_fixture():
    for dl in D.DICT_LENS:
        d = D.dictionary(dl)
        for v in (v for v in D.valid() if v["dict_len"] == dl):
            r, out = D.decode(v["bytes"], v["n"], d)
            assert r == v["n"] and D.sha(out) == v["sha256"] and out == D.record(v["size"], v["seed"]), v["name"]
            assert D.size_walk(v["bytes"], dl) == v["n"], v["name"]
            if v["n"] >= 12:
                assert D.decode(v["bytes"], v["n"] + 12, d) == (r, out), v["name"]           # the capacity is a bound (CJ_LZ4_SIZE_SLACK)
    for m in D.mutations():
        r, out = model_verdict(m, m["dict_len"])
        assert r == m["result"] and (r < 0 or D.sha(out) == m["sha256"]), m["name"]
    for h in D.hand():
        r, out = model_verdict(h, h["dict_len"])
        assert r == h["result"] and (r >= 0) == h["accepted"] and (r < 0 or D.sha(out) == h["sha256"]), h["name"]


def test_hand_written_streams_decode_to_what_they_say():
    by = {h["name"]: h for h in D.hand()}
    d4k, L = D.dictionary(4096), D.words(400, 77)
    out = D.decode_block(by["dict_then_periodic"]["bytes"], 47, d4k)
    head = L[:2] + d4k[-8:]
    assert out == head + (head * 5)[:32] + b"tail!"                                      # 8 bytes of dictionary, then period 10 from out + 0
    out = D.decode_block(by["dict_100_rest_200"]["bytes"], 325, d4k)
    head = L[:20] + d4k[-100:]
    assert out == head + (head * 2)[:200] + b"tail!"
    out = D.decode_block(by["dict_3000_rest_2000"]["bytes"], 5012, d4k)
    assert out == L[:7] + d4k[-3000:] + (L[:7] + d4k[-3000:])[:2000] + b"tail!"
    out = D.decode_block(by["first_match_one_byte_dict"]["bytes"], 13, D.dictionary(1))
    assert out == D.dictionary(1) * 8 + b"tail!"
    out = D.decode_block(by["above_64k_late_match_in_output"]["bytes"], by["above_64k_late_match_in_output"]["cap"], d4k)
    assert len(out) == 70115 and out[70:70070] == L[69:70] * 70000 and out[70090:70110] == out[70090 - 65535:70110 - 65535]
    # without its dictionary the same stream is refused, by the model's rule and by the plain size walk
    assert D.decode(by["first_match_into_dict"]["bytes"], 13, b"") == (D.CORRUPT, b"")
    assert D.size_walk(by["first_match_into_dict"]["bytes"], 0) == D.CORRUPT and D.size_walk(by["first_match_into_dict"]["bytes"], 7) == 13
    assert D.size_walk(by["offset_op_plus_dict_plus_1"]["bytes"], 7) == D.CORRUPT and D.size_walk(by["offset_op_plus_dict"]["bytes"], 7) == 16
    # only the last 64 KiB of a longer dictionary count
    assert D.size_walk(by["offset_65535_tail_of_70000"]["bytes"], 70000) == 18
    # the size prefix in front of the same streams
    for h in D.hand():
        pre = h["cap"].to_bytes(4, "little") + h["bytes"]
        assert D.decode(pre, h["cap"] + 3, D.dictionary(h["dict_len"]), prefix=True)[0] == h["result"], h["name"]
    assert D.decode(b"\x10\x00\x00\x00" + by["offset_op_plus_dict"]["bytes"], 15, D.dictionary(7), prefix=True)[0] == D.OUT_TOO_SMALL


def test_model_agrees_with_liblz4_on_the_fly():
    L = D.liblz4()
    if L is None:
        pytest.skip("liblz4 with LZ4_decompress_safe_usingDict is not installed")
    for dl in D.BATCH_DICT_LENS:
        d = D.dictionary(dl)
        for c in D.cases(dl):
            if c["name"] == "offset_0":
                continue                                                                 # the documented deviation: liblz4 reads it as a run
            r, out = D.lz4_decode_using_dict(L, c["bytes"], c["cap"], d)
            mr, mout = model_verdict(c, dl)
            assert (r < 0 and mr == D.CORRUPT) or (r == mr and out == mout), (c["name"], r, mr)
    # fresh seeded mutations, not in the fixture file
    import numpy as np
    rng = np.random.default_rng(5)
    vs = [v for v in D.valid() if v["size"] in (300, 4096)]
    for k in range(200):
        v = vs[int(rng.integers(0, len(vs)))]
        s = D.mutate(v["bytes"], int(rng.integers(0, len(v["bytes"]))), int(rng.integers(0, 256)))
        d = D.dictionary(v["dict_len"])
        r, out = D.lz4_decode_using_dict(L, s, v["n"], d)
        mr, mout = D.decode(s, v["n"], d)
        assert (r < 0 and mr == D.CORRUPT) or (r == mr and out == mout) or D.has_offset0(s, v["n"], d), (v["name"], k, r, mr)


def sim_lib():
    """tests/hostsim/sim_lz4_wave.cpp: lz4_wave_decode<true> (sim_lz4_dict_decode) and <false> (sim_lz4_wave_decode)"""
    L = C.CDLL(build_sim("sim_lz4_wave.cpp", os.path.join(SIM_DIR, "libsim_lz4_wave.so")))
    L.sim_lz4_dict_decode.restype = C.c_longlong
    L.sim_lz4_dict_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    L.sim_lz4_wave_decode.restype = C.c_longlong
    L.sim_lz4_wave_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_uint]
    return L


def test_kernels_block_decoder_on_the_host_agrees_with_the_model():
    """cramjam_amd/csrc/lz4_wave.hpp's lz4_wave_decode<true>, the function the kernel runs, compiled for the host (tests/hostsim/sim_lz4_wave.cpp:
    every copy bounds-checked, a violation is SIM_BOUNDS): every fixture stream at input alignments 0, 1 and 3 and dictionary alignments 0 and
    5 gives the model's verdict and bytes"""
    L = sim_lib()
    runs = 0
    for dl in D.BATCH_DICT_LENS:
        d = D.dictionary(dl)
        dbufs = []
        for md in (0, 5):
            b = (C.c_ubyte * (dl + 32))()
            base = C.addressof(b) + (-C.addressof(b) % 16) % 16
            C.memmove(base + md, d, dl)
            dbufs.append((b, base + md))
        for c in D.cases(dl):
            want_r, want = model_verdict(c, dl)
            s, cap = c["bytes"], c["cap"]
            for mis in (0, 1, 3):
                buf = (C.c_ubyte * (len(s) + 8))()
                assert C.addressof(buf) % 4 == 0
                C.memmove(C.addressof(buf) + mis, s, len(s))
                for _b, dptr in dbufs:
                    out = (C.c_ubyte * max(cap, 1))()
                    r = L.sim_lz4_dict_decode(C.addressof(buf) + mis, len(s), out, cap, dptr, dl)
                    assert r != SIM_BOUNDS, (c["name"], mis)
                    assert r == want_r and (r < 0 or bytes(out[:r]) == want), (c["name"], mis, r, want_r)
                    runs += 1
    assert runs >= 6 * (len(D.valid()) + len(D.mutations()) + len(D.hand()))


def test_encoder_model_with_the_dictionary_as_history():
    """what the GPU encoder is held to (tests/hostsim/enc2_linked_model.c with hist = the dictionary's tail): its streams decode with
    the model and with liblz4, need the dictionary, and beat liblz4 without one on word-like records"""
    from test_enc2_linked_model import linked_lib, model_linked
    M, L = linked_lib(), D.liblz4()
    for dl in D.DICT_LENS:
        d = D.dictionary(dl)
        for k, size in enumerate(n for n in D.RECORD_SIZES if n <= 65536):
            raw = D.words(size, 300 + k)
            s = model_linked(M, d, raw)
            assert D.decode(s, size, d) == (size, raw), (dl, size)
            assert D.size_walk(s, dl) == size
            if L is not None:
                assert D.lz4_decode_using_dict(L, s, size, d) == (size, raw), (dl, size)
    d = D.dictionary(65536)
    for size in (300, 4096, 16384):
        raws = [D.words(size, 900 + k) for k in range(8)]
        with_dict = sum(len(model_linked(M, d, r)) for r in raws)
        without = sum(len(model_linked(M, b"", r)) for r in raws)
        assert with_dict < 0.9 * without, (size, with_dict, without)
        if L is not None:
            assert with_dict < sum(len(D.lz4_compress_plain(L, r)) for r in raws), size


def test_argument_refusals_that_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    d = C.create_string_buffer(b"dictionary", 10)
    dev = lambda codec, op, flags, dp, dl: L.cj_dict_batch_device(None, codec, op, flags, 0, None, None, None, None, None, None, None, dp, dl, None)
    host = lambda codec, op, flags, dp, dl: L.cj_dict_batch_host(None, codec, op, flags, 0, None, None, None, None, None, dp, dl)
    for op in (0, 1):
        for call in (dev, host):
            assert call(N.CODEC_LZ4_BLOCK, op, 0, d, 10) == 0
            assert call(N.CODEC_LZ4_BLOCK, op, N.FLAG_LZ4_SIZE_PREFIX, d, 10) == 0
            assert call(N.CODEC_LZ4_BLOCK, op, 0, None, 0) == 0                           # no dictionary: the plain call
            assert call(N.CODEC_SNAPPY_RAW, op, 0, d, 10) == D.BAD_ARG                    # Snappy has no dictionaries
            assert call(N.CODEC_SNAPPY_RAW, op, 0, None, 0) == D.BAD_ARG
            assert call(N.CODEC_LZ4_BLOCK, op, 0, None, 10) == D.BAD_ARG                  # a null dictionary with a length
            for flags in (N.FLAG_FORCE_WAVE_PER_CHUNK, N.FLAG_FORCE_LANE_PER_CHUNK, N.FLAG_FORCE_LDS_PER_CHUNK, N.FLAG_BIG_CHUNKS, N.FLAG_CHUNKS_LE_16K, 2, 0x80000000):
                assert call(N.CODEC_LZ4_BLOCK, op, flags, d, 10) == D.BAD_ARG, flags      # the mapping overrides are refused
    for call in (dev, host):
        assert call(N.CODEC_LZ4_BLOCK, 2, 0, d, 10) == D.BAD_ARG
    for flags, want in ((0, 0), (1, 0), (0x100, D.BAD_ARG), (2, D.BAD_ARG)):
        assert L.cj_dict_batch_sizes_device(None, N.CODEC_LZ4_BLOCK, flags, 0, None, None, None, None, 10, None) == want
        assert L.cj_dict_batch_sizes_host(None, N.CODEC_LZ4_BLOCK, flags, 0, None, None, None, 10) == want
    assert L.cj_dict_batch_sizes_device(None, N.CODEC_SNAPPY_RAW, 0, 0, None, None, None, None, 10, None) == D.BAD_ARG
    assert L.cj_dict_batch_sizes_host(None, N.CODEC_SNAPPY_RAW, 0, 0, None, None, None, 10) == D.BAD_ARG
    # a batch without its pointers
    assert L.cj_dict_batch_device(None, 0, 0, 0, 3, None, None, None, None, None, None, None, d, 10, None) == D.BAD_ARG
    assert L.cj_dict_batch_host(None, 0, 0, 0, 3, None, None, None, None, None, d, 10) == D.BAD_ARG
    for flags in (0, N.FLAG_LZ4_SIZE_PREFIX):
        for dict_len in (10, 0):
            assert L.cj_dict_batch_sizes_device(None, 0, flags, 3, None, None, None, None, dict_len, None) == D.BAD_ARG
            assert L.cj_dict_batch_sizes_host(None, 0, flags, 3, None, None, None, dict_len) == D.BAD_ARG
    assert L.cj_debug_dict_stage_budget(0) == 1 << 30
    # the Python keyword: a Snappy call has none
    from cramjam_amd import batch
    with pytest.raises(TypeError):
        batch.snappy_decompress_raw_many([b"\x00"], dictionary=b"abc")
