"""The DEFLATE kernel on streams zlib never writes (tests/deflate_synth.py: every family; tests/golden/golden_deflate_others.*: libdeflate's
and zopfli's streams and their mutations): per wrapper all of them, shuffled so that the four wavefronts of a workgroup hold cases of
different families and lengths, through cj_deflate_batch_device with 64 guard bytes of 0xA5 around every slot and through
batch.deflate_decompress_many; batches of 1, 3 and 5; capacities n - 1 and 0 and each case's cuts (a literal run cut at 62..65 literals,
a stored block at its edges) against zlib's live verdict at that capacity; the size query, device and host.  The host build of the same
decoder passes all of this in tests/test_deflate_synth_model.py: what is new here is the wavefront's own code (the register window over
the input, the literals kept in the lanes, the byte movers, the order between lanes)."""
import numpy as np
import pytest

import deflate_cases as D
import deflate_synth as S
import device_batch as DB
from test_deflate_gpu import eng  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu
_cache = {}


def _cases(wrap):
    """[dict(name, bytes, result, out, cap, cuts, family)] of one wrapper in a fixed shuffled order; result / out: zlib's, at capacity cap"""
    if wrap not in _cache:
        cs = []
        for c in S.cases(wrap):
            n = len(c.expected) if c.expected is not None else 300
            r, out = D.verdict(wrap, c.stream, n)
            assert r == (n if c.expected is not None else D.CORRUPT)
            cs.append(dict(name=c.name, bytes=c.stream, result=r, out=out, cap=n, cuts=c.cuts, family=next(f for f in ("codes", "headers", "matches", "literal_runs", "stored", "blocks") if f in c.features)))
        for c in D.others() + D.other_mutations():
            if c["wrap"] == wrap:
                r, out = D.verdict(wrap, c["bytes"], c["cap"])
                assert r == c["result"] and (r < 0 or D.sha(out) == c["sha256"])
                cs.append(dict(name=c["name"], bytes=c["bytes"], result=r, out=out, cap=c["cap"], cuts=(), family="others"))
        cs = [cs[k] for k in np.random.default_rng(wrap + 11).permutation(len(cs))]
        # early leavers as a workgroup's FIRST wavefront, beside three that run on: streams cut inside the wrapper's header
        for j, k in enumerate((0, 1, 3, 9, 11, 2, 5, 0)):
            c = cs[24 * j + 1]
            r, out = D.verdict(wrap, c["bytes"][:k], c["cap"])
            assert r < 0
            cs.insert(24 * j, dict(c, name="%s_cut_%d" % (c["name"], k), bytes=c["bytes"][:k], result=r, out=out, cuts=(), family="cut"))
        _cache[wrap] = cs
    return _cache[wrap]


def _check(part, caps, res, out, ooff, want=None):
    for i, c in enumerate(part):
        r, raw = want[i] if want is not None else (c["result"], c["out"])
        assert res[i] == r, (c["name"], int(caps[i]), int(res[i]), r)
        assert r < 0 or out[ooff[i]:ooff[i] + r].tobytes() == raw, (c["name"], int(caps[i]))
    bad = DB.guards_intact(out, ooff, caps)
    assert bad is None, part[bad]["name"]


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_device_batch_over_all_synthesized_and_other_encoders_streams(eng, wrap):
    e, N = eng
    cs = _cases(wrap)
    # (the mutated streams of the other encoders are raw and zlib; the gzip batch has the synthesized refusal and the cut headers)
    assert len(cs) >= 200 and sum(1 for c in cs if c["result"] < 0) >= (9 if wrap == D.GZIP else 20)
    # neighbours in a workgroup differ: most groups of four hold more than one family
    assert sum(1 for k in range(0, len(cs) - 3, 4) if len({c["family"] for c in cs[k:k + 4]}) > 1) > 0.6 * (len(cs) // 4)
    for part in (cs[:1], cs[1:4], cs[4:9], cs):                       # 1, 3 and 5 chunks: idle wavefronts in the last workgroup
        caps = [c["cap"] for c in part]
        res, out, ooff = D.device_call(e, N, wrap, [c["bytes"] for c in part], caps)
        _check(part, caps, res, out, ooff)


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_host_batch_over_all_synthesized_and_other_encoders_streams(wrap):
    from cramjam_amd import batch
    cs = _cases(wrap)
    for part in (cs[:1], cs[1:4], cs[4:9], cs):
        res, outs = batch.deflate_decompress_many([c["bytes"] for c in part], output_lens=[c["cap"] for c in part], wrapper=D.WRAP_NAME[wrap])
        for c, r, o in zip(part, res, outs):
            assert r == c["result"] and len(o) == max(r, 0) and (r < 0 or bytes(o) == c["out"]), (c["name"], r, c["result"])


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_capacities_one_less_and_zero(eng, wrap):
    """zlib's live verdict at that capacity; nothing outside a slot"""
    e, N = eng
    cs = [c for c in _cases(wrap) if c["name"] not in D.DIVERGES_FROM_ZLIB]
    chunks = [c["bytes"] for c in cs]
    exact = [c["result"] if c["result"] >= 0 else c["cap"] for c in cs]
    for caps in ([max(x - 1, 0) for x in exact], [0] * len(cs)):
        res, out, ooff = D.device_call(e, N, wrap, chunks, caps)
        _check(cs, caps, res, out, ooff, [D.verdict(wrap, c["bytes"], cap) for c, cap in zip(cs, caps)])


@pytest.mark.parametrize("family", ("literal_runs", "stored"))
@pytest.mark.parametrize("wrap", D.WRAPS)
def test_cut_capacities(eng, wrap, family):
    """a literal run ended by the capacity at 62, 63, 64 and 65 literals; a stored block that ends 0, 1 and 2 bytes beyond the capacity or
    begins there (the one byte kept behind the capacity): one chunk per (case, capacity), zlib's live verdict"""
    e, N = eng
    todo = [(c, cap) for c in _cases(wrap) if c["family"] == family for cap in c["cuts"]]
    assert len(todo) >= (20 if family == "literal_runs" else 200) * (1 if wrap == D.RAW else 0.2)
    todo = [todo[k] for k in np.random.default_rng(5).permutation(len(todo))]
    part, caps = [t[0] for t in todo], [t[1] for t in todo]
    want = [D.verdict(wrap, c["bytes"], cap) for c, cap in todo]
    assert D.OUT_TOO_SMALL in {w[0] for w in want}
    res, out, ooff = D.device_call(e, N, wrap, [c["bytes"] for c in part], caps)
    _check(part, caps, res, out, ooff, want)
    from cramjam_amd import batch
    res, outs = batch.deflate_decompress_many([c["bytes"] for c in part], output_lens=caps, wrapper=D.WRAP_NAME[wrap])
    for c, cap, w, r, o in zip(part, caps, want, res, outs):
        assert r == w[0] and (r < 0 or bytes(o) == w[1]), (c["name"], cap, r, w[0])


@pytest.mark.parametrize("wrap", D.WRAPS)
def test_size_query_device_and_host(eng, wrap):
    e, N = eng
    from cramjam_amd import batch
    cs = _cases(wrap)
    chunks = [c["bytes"] for c in cs]
    want = [D.size_verdict(wrap, s) for s in chunks]
    res, _, _ = D.device_call(e, N, wrap, chunks, [0] * len(cs), sizes=True)
    for c, r, w in zip(cs, res, want):
        assert int(r) == w, (c["name"], int(r), w)
    assert batch.deflate_sizes(chunks, wrapper=D.WRAP_NAME[wrap]) == want
