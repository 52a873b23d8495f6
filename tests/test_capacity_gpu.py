"""The capacity sweep on the GPU (tests/capacity_cases.py: ~6 000 - 8 000 (stream, capacity) chunks per body, expected values from the CPU
oracle) through every LZ4 and Snappy decoder path of a device-resident batch: one wavefront / one lane per chunk, the workgroup decoder
behind the parse kernel and with the parse inside it, the default pipeline below and above CJ_FUSED_MAX_CHUNKS, the 32 KiB and 16 KiB
windows with each placement of the parse, big chunks, the LZ4 size prefix, the shared dictionary.

Slots by tests/device_batch.py: inputs packed at every misalignment, 64 guard bytes of 0xA5 on both sides of every output slot, the
whole output filled before the call.  For every chunk: the oracle's result (LZ4: any refusal is CJ_E_CORRUPT; Snappy and the size prefix:
the oracle's code), the oracle's bytes in [0, result), both guards intact — accepted or refused —, and [result, cap) untouched where the
chunk was accepted (a refused chunk may have written inside its own slot)."""
import ctypes as C
import functools

import pytest

import capacity_cases as K
import lz4_dict_model as D
import test_spec_parse_model as M
from capacity_cases import PATHS
from cramjam_amd import _native as N

pytestmark = pytest.mark.gpu
LZ4, SN, DEC = N.CODEC_LZ4_BLOCK, N.CODEC_SNAPPY_RAW, N.OP_DECOMPRESS
PROFILE = 0x1000                                  # CJ_FLAG_DEBUG_PROFILE: the debug counters count
WAVE, LANE, LDS = N.FLAG_FORCE_WAVE_PER_CHUNK, N.FLAG_FORCE_LANE_PER_CHUNK, N.FLAG_FORCE_LDS_PER_CHUNK
PK, FUSED = N.FLAG_FORCE_PARSE_KERNEL, N.FLAG_FORCE_FUSED_PARSE


@pytest.fixture(scope="module")
def eng():
    e = N.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("flags,win", PATHS)
def test_lz4_capacity_sweep(eng, flags, win):
    for body in K.lz4_bodies(win):
        K.run_and_check(eng, LZ4, flags, ("lz4", body), K.lz4_cases(body))


@pytest.mark.parametrize("flags,win", PATHS)
def test_snappy_declared_length_and_capacity_sweep(eng, flags, win):
    for body in K.SNAPPY_BODIES:
        K.run_and_check(eng, SN, flags, ("snappy", body), K.snappy_cases(body))


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_default_pipeline_above_the_one_kernel_limit(eng, codec):
    """16 384 + 41 chunks: the parse kernel in front of the workgroup decoder, chosen by the engine"""
    cs = K.lz4_cases("b") if codec == LZ4 else K.snappy_cases("b")
    n = 16384 + 41
    assert len(cs) < n
    K.run_and_check(eng, codec, 0, ("above", codec), [cs[i % len(cs)] for i in range(n)])


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_big_chunks_capacity_sweep(eng, codec):
    """the ~100 KiB streams under CJ_FLAG_BIG_CHUNKS: around U and around 32 768, 65 536 (below it the chunk takes the small-chunk path: intended)
    and 98 304 (the slabs' boundaries)"""
    K.run_and_check(eng, codec, N.FLAG_BIG_CHUNKS, ("big", codec), K.big_cases("lz4" if codec == LZ4 else "snappy"))


@pytest.mark.parametrize("flags", [pytest.param(WAVE, id="wave-per-chunk"), pytest.param(LDS | FUSED, id="lds+fused-parse")])
def test_lz4_size_prefix_sweep(eng, flags):
    """the PREFIX takes the capacity's place (out_cap = U + 64): the prologue's codes for a prefix above out_cap, negative or too big"""
    for body in K.LZ4_BODIES[:2]:
        cs = K.lz4_prefix_cases(body)
        assert {-4, -5, -6, -7} <= {c["result"] for c in cs}
        K.run_and_check(eng, LZ4, flags | N.FLAG_LZ4_SIZE_PREFIX, ("prefix", body), cs)


def test_lz4_dictionary_capacity_sweep(eng):
    """bodies whose first twenty matches reach into the dictionary (tests/lz4_dict_model.py decides)"""
    for body in K.LZ4_BODIES:
        cs = K.lz4_dict_cases(body)
        assert sum(c["result"] >= 0 for c in cs) >= 150
        K.run_and_check(eng, LZ4, 0, ("dict", body), cs, dictionary=D.dictionary(4096))


@functools.lru_cache(maxsize=None)
def _elements(at, b):
    """elements a walk of the true path reads before it ends or meets a malformed one (what the in-kernel parse counts)"""
    n = ip = 0
    while True:
        ok, _, _, _, nxt, last = at(b, ip, len(b))
        if not ok: return n
        n += 1
        if last or nxt == M.END: return n
        ip = nxt


def _reaches_the_in_kernel_checks(codec, c):
    """lz4_decode_lds.hip (kFused prologue) + lds_shared.hpp fused_parse: a chunk is counted in cj_debug_fused_parse_paths when the prologue
    does not hand it to the wave kernel (no room / a declared length of 0, above out_cap or above the window; no input) and its walk
    finds 256 .. 16 384 elements — BEFORE the capacity rules give their verdict, so refused chunks count as well"""
    blob, cap = c["bytes"], c["cap"]
    if codec == LZ4:
        return cap > 0 and cap <= 65536 and 0 < len(blob) <= 65504 and 256 <= _elements(M.seq_at, blob) <= 16384
    hdr = next(i for i, x in enumerate(blob) if x < 0x80) + 1
    dn = sum((x & 0x7f) << (7 * i) for i, x in enumerate(blob[:hdr]))
    return 0 < dn <= min(cap, 65536) and 0 < len(blob) - hdr <= 65504 and 256 <= _elements(M.snappy_at, blob[hdr:]) <= 16384


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_accepted_chunks_are_decoded_by_the_workgroup_decoder(eng, codec):
    """On FORCE_LDS | FORCE_FUSED_PARSE with the debug counters on: the workgroup decoder completes exactly as many chunks as the oracle
    accepts (cj_debug_lds_phase_cycles, word 5: one per chunk streamed out of the window) — none of them was quietly left to the wave
    kernel.  cj_debug_fused_parse_paths counts at the ENTRY of the parse's capacity checks, so its sum is not the accepted count: it is
    the number of chunks that reach those checks, accepted or refused (the rule: _reaches_the_in_kernel_checks) — every refusal of the
    sweep beyond the prologue's was therefore made by Lz4Grammar / SnappyGrammar::check inside the decoder kernel."""
    L = N.lib()
    paths, cyc = (C.c_ulonglong * 3)(), (C.c_ulonglong * 16)()
    for body in (K.LZ4_BODIES if codec == LZ4 else K.SNAPPY_BODIES):
        cs = K.lz4_cases(body) if codec == LZ4 else K.snappy_cases(body)
        accepted = sum(c["result"] >= 0 for c in cs)
        reached = sum(_reaches_the_in_kernel_checks(codec, c) for c in cs)
        assert accepted >= 150 and reached >= accepted + 3000
        assert L.cj_debug_fused_parse_paths(paths, 1) == 0 and L.cj_debug_lds_phase_cycles(cyc, 1) == 0
        K.run_and_check(eng, codec, LDS | FUSED | PROFILE, ("lz4" if codec == LZ4 else "snappy", body), cs)
        assert L.cj_debug_fused_parse_paths(paths, 0) == 0 and L.cj_debug_lds_phase_cycles(cyc, 0) == 0
        assert sum(paths) == reached, (body, list(paths), reached)
        assert cyc[5] == accepted, (body, cyc[5], accepted)
