"""The Zstandard kernel on streams libzstd never writes (tests/zstd_synth.py: every family, 600 seeded single-bit flips and the Huffman grid's own flips) against the
RECORDED verdicts of libzstd (tests/golden/golden_zstd_synth.json; libzstd is not called here, the streams are made again from their
seeds and held to their recorded digests): all of them in one shuffled batch through cj_zstd_batch_device at capacities exact, + 64, - 1
and 0 with 64 guard bytes of 0xA5 around every slot, the four wavefronts of a workgroup on different families and chunks refused inside
their frame header leading several workgroups; the host entry and the size query; batches of 1, 3 and 5; the slot budget at 3 slots.
The host build of the same decoder passes all of this in tests/test_zstd_synth_model.py: what is new here is the wavefront's own code."""
import json
import os

import numpy as np
import pytest

import zstd_cases as Z
import zstd_synth as S
from conftest import ROOT
from test_zstd_gpu import eng  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu
_cache = []


def _cases():
    """every synthesized case and recorded flip as zstd_cases.Case (tags: its family), in a fixed shuffled order"""
    if not _cache:
        rec = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_zstd_synth.json")))["cases"]
        made = [(c.name, c.stream, c.family) for c in S.cases()] + [(f[0], f[2], f[1]) for f in S.flips(600) + S.grid_flips()]
        assert len(rec) == len(made)
        cs = []
        for m, (name, stream, family) in zip(rec, made):
            assert m[0] == S.digest(stream), name                                            # the generator has not drifted
            cs.append(Z.Case(name, stream, m[1], m[2], m[3] if len(m) > 3 else None, {family}))
        cs = [cs[k] for k in np.random.default_rng(23).permutation(len(cs))]
        # early leavers as a workgroup's FIRST wavefront, beside three that run on: chunks refused inside their frame header
        early = [k for k, c in enumerate(cs) if c.name.startswith(("frame_reserved_bit", "frame_window_0xb0", "frame_window_0xf8"))]
        assert len(early) >= 6
        for j, k in enumerate(early):
            cs[40 * j], cs[k] = cs[k], cs[40 * j]
        for j in range(len(early)):
            assert cs[40 * j].verdicts[1] == Z.E_HEADER and all(c.verdicts[1] != Z.E_HEADER for c in cs[40 * j + 1:40 * j + 4])
        _cache.extend(cs)
    return _cache


def test_the_shuffle_mixes_families_within_a_workgroup():
    cs = _cases()
    assert len(cs) >= 1400 and sum(1 for c in cs if not c.accepted) >= 300
    assert sum(1 for k in range(0, len(cs) - 3, 4) if len({next(iter(c.tags)) for c in cs[k:k + 4]}) > 1) > 0.8 * (len(cs) // 4)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_all_cases_and_flips_in_one_batch_at_four_capacities(eng, which):
    e, N = eng
    cs = _cases()
    caps = [Z.capacities(c.cap)[which] for c in cs]
    res, out, ooff = Z.device_call(e, N, [c.stream for c in cs], caps)
    Z.check_batch(cs, which, res, out, ooff, caps, S.digest)


def test_host_entry_and_size_query():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    cs = _cases()
    chunks = [c.stream for c in cs]
    res, outs = batch._run(N.ZSTD_FRAMES, N.OP_DECOMPRESS, 0, chunks, [c.cap for c in cs], None, None, N.ZSTD)
    for c, r, o in zip(cs, res, outs):
        assert r == c.verdicts[0] and len(o) == max(r, 0) and (r < 0 or S.digest(o) == c.sha), (c.name, r)
    sizes = batch.zstd_sizes(chunks)
    for c, q in zip(cs, sizes):
        d = c.verdicts[1]                                      # the decoder with room to spare
        assert q == d or d == Z.E_OUT_TOO_SMALL or (d < 0 and Z.size_query_may_miss(c.stream, d)), (c.name, q, d)
    res, outs = batch.zstd_decompress_many(chunks)
    for c, q, r, o in zip(cs, sizes, res, outs):
        if q < 0:
            assert r == q and len(o) == 0, c.name
        elif c.accepted:
            assert r == c.verdicts[0] and S.digest(o) == c.sha, c.name
        elif c.verdicts[1] >= 0:                                  # a flip that decodes to more than its case's capacity: the query's size
            assert r == c.verdicts[1] == q, (c.name, r)
        elif c.verdicts[1] != Z.E_OUT_TOO_SMALL:
            assert r < 0, (c.name, r)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_batches_that_leave_wavefronts_idle(eng, n):
    e, N = eng
    small = [c for c in _cases() if c.cap < 8192]
    for start in (0, 7, 100, 333):
        part = small[start:start + n]
        caps = [c.cap for c in part]
        res, out, ooff = Z.device_call(e, N, [c.stream for c in part], caps)
        Z.check_batch(part, 0, res, out, ooff, caps, S.digest)


def test_slot_budget_of_three_slots_over_ten_huffman_cases(eng):
    e, N = eng
    part = [c for c in _cases() if c.name.startswith(("huf_log", "huf_treeless", "nc_w_"))]
    part = [c for c in part if c.accepted][:7] + [c for c in part if not c.accepted][:3]
    assert len(part) == 10
    caps = [c.cap for c in part]
    slot = 131072 + 32
    prev = N.lib().cj_debug_zstd_slot_budget(3 * slot)
    try:
        res, out, ooff = Z.device_call(e, N, [c.stream for c in part], caps)
    finally:
        assert N.lib().cj_debug_zstd_slot_budget(prev) == 3 * slot
    Z.check_batch(part, 0, res, out, ooff, caps, S.digest)
