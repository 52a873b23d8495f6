"""Zstandard batches on the GPU (cj_zstd_batch_* / cramjam_amd.batch.zstd_*) against the RECORDED verdicts of libzstd
(tests/golden/golden_zstd.*; libzstd itself is not needed here): every fixture, hand-written stream and mutation in one shuffled batch
at capacities exact, + 64, - 1 and 0 with 64 guard bytes of 0xA5 around every slot and nothing written behind a result; batches of
1, 3, 4, 5 and 257 chunks; the slot budget shrunk to 3 slots; the size query and the decode laid out from it; out= and devices=[0, 0];
torch tensors on a side stream."""
import os

import numpy as np
import pytest

import device_batch as DB
import zstd_cases as Z
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd import _native as N
    from cramjam_amd.batch import _engine
    return _engine(0), N


def _shuffled():
    cs = [c for c in Z.load_cases() if c.name not in Z.DIVERGES_FROM_ZSTD]
    return [cs[k] for k in np.random.default_rng(7).permutation(len(cs))]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_all_cases_in_one_batch_at_four_capacities(eng, which):
    e, N = eng
    cs = _shuffled()
    caps = [Z.capacities(c.cap)[which] for c in cs]
    res, out, ooff = Z.device_call(e, N, [c.stream for c in cs], caps)
    Z.check_batch(cs, which, res, out, ooff, caps)


def test_all_cases_in_one_host_batch():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    cs = _shuffled()
    res, outs = batch._run(N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, [c.stream for c in cs], [c.cap for c in cs], None, None, N.ZSTD)
    for c, r, o in zip(cs, res, outs):
        assert r == c.verdicts[0] and len(o) == max(r, 0) and (r < 0 or Z.sha(o) == c.sha), (c.name, r)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_batch_edges_of_four_wavefronts_per_workgroup(eng, n):
    e, N = eng
    cs = _shuffled()
    ok, bad = [c for c in cs if c.accepted and c.cap < 8192], [c for c in cs if not c.accepted]
    part = [(bad if i % 3 == 1 else ok)[i % 50] for i in range(n)]          # refused chunks between accepted ones
    caps = [c.cap for c in part]
    res, out, ooff = Z.device_call(e, N, [c.stream for c in part], caps)
    Z.check_batch(part, 0, res, out, ooff, caps)


def test_slot_budget_of_three_slots_over_ten_streams(eng):
    e, N = eng
    part = [c for c in _shuffled() if c.accepted and "lit:huf4" in c.tags][:5] + [c for c in _shuffled() if c.accepted and c.name.startswith("mut_")][:5]
    assert len(part) == 10
    caps = [c.cap for c in part]
    slot = 131072 + 32
    prev = N.lib().cj_debug_zstd_slot_budget(3 * slot)
    try:
        res, out, ooff = Z.device_call(e, N, [c.stream for c in part], caps)
    finally:
        assert N.lib().cj_debug_zstd_slot_budget(prev) == 3 * slot
    Z.check_batch(part, 0, res, out, ooff, caps)
    res2, out2, _ = Z.device_call(e, N, [c.stream for c in part], caps)
    assert list(res2) == list(res) and (out2 == out).all()


def test_five_frames_at_a_budget_below_one_slot(eng):
    """a budget of one byte is one slot: five slices of one frame each — the five accepted frames whose content is nearest 70 KB —
    every output what the same call writes at the default budget"""
    e, N = eng
    L = N.lib()
    default = 4096 * (131072 + 32)
    part = sorted((c for c in _shuffled() if c.accepted and not c.name.startswith("mut_")), key=lambda c: (abs(c.cap - 70000), c.name))[:5]
    assert all(60000 < c.cap < 140000 for c in part)
    caps = [c.cap for c in part]
    res0, out0, _ = Z.device_call(e, N, [c.stream for c in part], caps)
    assert L.cj_debug_zstd_slot_budget(1) == default                  # (the setter returns the previous value)
    try:
        res, out, ooff = Z.device_call(e, N, [c.stream for c in part], caps)
    finally:
        assert L.cj_debug_zstd_slot_budget(0) == 1                    # 0: back to the default
    assert L.cj_debug_zstd_slot_budget(0) == default
    Z.check_batch(part, 0, res, out, ooff, caps)
    assert list(res) == list(res0) and (out == out0).all()


def test_size_query_then_the_public_calls(eng):
    e, N = eng
    from cramjam_amd import batch
    cs = _shuffled()
    chunks = [c.stream for c in cs]
    sizes, _, _ = Z.device_call(e, N, chunks, [0] * len(cs), sizes=True)
    assert batch.zstd_sizes(chunks) == [int(s) for s in sizes]
    for c, q in zip(cs, sizes):
        d = c.verdicts[1]
        assert q == d or d == Z.E_OUT_TOO_SMALL or (d < 0 and Z.size_query_may_miss(c.stream, d)), (c.name, int(q), d)
    by = {c.name: int(q) for c, q in zip(cs, sizes)}
    assert by["hand_bad_offset"] == by["hand_literal_overrun"] == Z.E_CORRUPT
    res, outs = batch.zstd_decompress_many(chunks)
    buf = bytearray(b"\xa5" * (sum(max(int(s), 0) for s in sizes) + 16))
    res2, views = batch.zstd_decompress_many(chunks, out=buf)
    res3, outs3 = batch.zstd_decompress_many(chunks, devices=[0, 0])
    assert list(res) == list(res2) == list(res3)
    for c, q, r, o, v, o3 in zip(cs, sizes, res, outs, views, outs3):
        if q < 0:
            assert r == q and len(o) == 0, c.name
        elif c.accepted:
            assert r == c.verdicts[0] and Z.sha(o) == c.sha and bytes(v) == bytes(o) == bytes(o3), c.name
        else:
            assert r < 0, (c.name, r)
    assert bytes(buf[-16:]) == b"\xa5" * 16
    assert batch.zstd_sizes([]) == [] and batch.zstd_sizes([b""]) == [0]


def test_device_entries_on_torch_tensors_on_a_side_stream():
    """the device-resident calls on torch tensors with sync=False, in a child that imports torch BEFORE cramjam_amd"""
    DB.run_child(os.path.join(ROOT, "tests", "zstd_torch_child.py"), "zstd: ok", 600)
