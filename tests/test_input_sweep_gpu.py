"""The input sweep on the GPU (tests/input_cases.py: where the input ends, the offset at its edges, the overlap grid; expected values from
the CPU oracle) through every LZ4 and Snappy decoder path of a device-resident batch — the capacity sweep's paths and its harness
(tests/device_batch.py: inputs at every misalignment, 64 guard bytes of 0xA5 around every output slot, the whole output filled before
the call, the oracle's result and bytes, [result, cap) untouched where the chunk was accepted).  What lies behind a cut's in_len is the
case's own `after`: the stream's continuation, or 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest

import capacity_cases as K
import device_batch as DB
import input_cases as I
import lz4_dict_model as D
from capacity_cases import PATHS, lz4_bodies as _lz4_bodies, run_and_check as _run_and_check
from cramjam_amd import _native as N
from test_capacity_gpu import eng  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu
LZ4, SN, LDS, FUSED, PROFILE = N.CODEC_LZ4_BLOCK, N.CODEC_SNAPPY_RAW, N.FLAG_FORCE_LDS_PER_CHUNK, N.FLAG_FORCE_FUSED_PARSE, 0x1000
ABOVE = 16384 + 41                                 # chunks: above CJ_FUSED_MAX_CHUNKS


@pytest.mark.parametrize("flags,win", PATHS)
def test_lz4_input_end_sweep(eng, flags, win):
    for body in _lz4_bodies(win):
        _run_and_check(eng, LZ4, flags, ("in-a-lz4", body), I.a_lz4_cases(body))


@pytest.mark.parametrize("flags,win", PATHS)
def test_snappy_input_end_sweep(eng, flags, win):
    for body in K.SNAPPY_BODIES:
        _run_and_check(eng, SN, flags, ("in-a-snappy", body), I.a_snappy_cases(body))


@pytest.mark.parametrize("flags,win", PATHS)
def test_offset_edges(eng, flags, win):
    """LZ4 and Snappy (every copy form), and the Snappy preamble's forms"""
    _run_and_check(eng, LZ4, flags, "in-b-lz4", [c for b in K.LZ4_BODIES[:2] for c in I.b_lz4_cases(b)])
    _run_and_check(eng, SN, flags, "in-b-snappy", [c for b in K.SNAPPY_BODIES for c in I.b_snappy_cases(b)] + I.b_preamble_cases())


@pytest.mark.parametrize("flags,win", PATHS)
def test_overlap_grid(eng, flags, win):
    """every (period, length) pair at every destination alignment, in the streams dealt for this path's window"""
    _run_and_check(eng, LZ4, flags, ("in-c-lz4", win), I.c_lz4_cases(win))
    _run_and_check(eng, SN, flags, ("in-c-snappy", win), I.c_snappy_cases(win))


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_default_pipeline_above_the_one_kernel_limit(eng, codec):
    """16 384 + 41 chunks, the parse kernel in front of the workgroup decoder: the 16 KiB grid's streams, and the cuts of body b"""
    for name, cs in (("c", I.c_lz4_cases(16384) if codec == LZ4 else I.c_snappy_cases(16384)), ("a", I.a_lz4_cases("b") if codec == LZ4 else I.a_snappy_cases("b"))):
        assert len(cs) < ABOVE
        _run_and_check(eng, codec, 0, ("in-above", name, codec), [cs[i % len(cs)] for i in range(ABOVE)])


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_big_chunks(eng, codec):
    """the ~100 KiB streams under CJ_FLAG_BIG_CHUNKS: cuts at the end and around the elements that cross 32 768, 65 536 and 98 304, offsets
    of 65 534 and 65 535 (Snappy: 65 536, ms and ms + 1 in the 4-byte form) behind 65 536 and 98 304, and overlapping matches of 66 and
    600 bytes that begin 1, 7, 8 and 33 bytes before each boundary"""
    name = "lz4" if codec == LZ4 else "snappy"
    _run_and_check(eng, codec, N.FLAG_BIG_CHUNKS, ("in-big", name), I.a_big_cases(name) + I.b_big_cases(name))
    _run_and_check(eng, codec, N.FLAG_BIG_CHUNKS, ("in-big-c", name), I.c_big_cases(name))


def test_dictionary_offsets_and_overlaps(eng):
    """cj_dict_batch_device: offsets up to the dictionary's first byte and one beyond; the grid with its first forty matches per stream
    beginning inside the dictionary's end (tests/lz4_dict_model.py decides)"""
    d = D.dictionary(I.DICT_LEN)
    cs = [c for b in K.LZ4_BODIES[:2] for c in I.b_dict_cases(b)]
    assert sum(c["result"] < 0 for c in cs) >= len(cs) // 8
    _run_and_check(eng, LZ4, 0, "in-b-dict", cs, dictionary=d)
    _run_and_check(eng, LZ4, 0, "in-c-dict", I.c_dict_cases(), dictionary=d)


def _sizes(eng, codec, key, cases):
    """cj_batch_sizes_device over the cases' inputs as the harness packs them (`after` behind every in_len)"""
    (blob, off, lens), want = DB.case_pack(key, cases), DB.case_slots(key, cases)[4]
    n = len(cases)
    d_in, d_meta = eng.alloc(blob.nbytes), eng.alloc(3 * 8 * n + 128)
    try:
        eng.h2d(d_in, blob)
        guard = np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64)
        eng.h2d(d_meta, np.concatenate([off, lens, guard, np.zeros(n, np.uint64), guard]))
        res = d_meta + 8 * (2 * n + 8)
        N.check(N.lib().cj_batch_sizes_device(eng.h, codec, 0, n, d_in, d_meta, d_meta + 8 * n, res, None))
        eng.sync()
        got = eng.d2h(d_meta + 8 * 2 * n, 8 * (n + 16), "int64")
    finally:
        eng.free(d_in); eng.free(d_meta)
    assert (got[:8].view(np.uint64) == guard).all() and (got[8 + n:].view(np.uint64) == guard).all(), "guard words around result were written"
    bad = np.nonzero(got[8:8 + n] != want)[0]
    assert len(bad) == 0, (len(bad), [(cases[i]["stream"], cases[i].get("in_len"), cases[i].get("kind"), cases[i].get("off"), cases[i].get("form"), int(got[8 + i]), int(want[i])) for i in bad[:6]])


def test_raw_lz4_size_query_on_the_cuts_and_offsets(eng):
    cs = I.size_cases()
    assert sum(c["result"] >= 0 for c in cs) >= 100
    _sizes(eng, LZ4, "in-sizes-lz4", cs)


def test_snappy_header_size_query_on_the_preambles(eng):
    cs = [dict(c, cap=0, result=c["size"], out=b"") for c in I.b_preamble_cases()]
    _sizes(eng, SN, "in-sizes-snappy", cs)
    L = N.lib()
    for c in cs:
        assert L.cj_snappy_raw_decompress_len(c["bytes"], len(c["bytes"])) == c["size"], c["form"]


@pytest.mark.parametrize("codec", [LZ4, SN])
def test_the_workgroup_decoder_completes_every_overlap_chunk(eng, codec):
    """On FORCE_LDS | FORCE_FUSED_PARSE with the debug counters on (as test_accepted_chunks_are_decoded_by_the_workgroup_decoder): one
    chunk streamed out of the window per family-C stream — the grid reaches lds_copy_serial and the long-run copy; nothing is handed to
    the wave kernel."""
    L = N.lib()
    cyc = (C.c_ulonglong * 16)()
    cs = I.c_lz4_cases(65536) if codec == LZ4 else I.c_snappy_cases(65536)
    assert all(c["result"] == c["U"] for c in cs)
    assert L.cj_debug_lds_phase_cycles(cyc, 1) == 0
    _run_and_check(eng, codec, LDS | FUSED | PROFILE, ("in-c-lz4" if codec == LZ4 else "in-c-snappy", 65536), cs)
    assert L.cj_debug_lds_phase_cycles(cyc, 0) == 0
    assert cyc[5] == len(cs), (cyc[5], len(cs))
