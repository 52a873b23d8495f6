"""The capacity sweep on the CPU (tests/capacity_cases.py): the builder's streams mean what was meant; the phase model of
tests/test_spec_parse_model.py (seq_at + lz4_check, snappy_at + snappy_check — the kernels' Lz4Grammar / SnappyGrammar restated) gives
the oracle's verdict and size on every (stream, capacity) case; the system liblz4, where it loads, agrees with the oracle on the tails
of 5 or more literals; and the sweep is not hollow: both verdicts occur on both sides of the decoded size.

liblz4 is NOT the reference on tails of 0 .. 4 literals: its fast loop (1.9.3 measured) accepts streams whose last match is followed by
fewer than 8 input bytes once the capacity is U or more, which its own safe loop and the oracle (the 1.10.0 safe decoder's
rules, `rem_in < lit + 8` = last sequence) refuse."""
import ctypes as C

import pytest

import capacity_cases as K
import lz4_dict_model as D
import oracle
import test_spec_parse_model as M


def test_every_stream_decodes_to_its_intended_bytes_with_room_to_spare():
    """at capacity U + 64 — the streams whose tail breaks the input-side end rule (fewer than 8 bytes behind the last match's literals)
    are refused there, as at every capacity"""
    n = 0
    for body in K.LZ4_BODIES:
        for s in K.lz4_streams(body):
            r, o = oracle.lz4_decompress_raw(s["bytes"], s["U"] + 64)
            assert (r, o) == ((s["U"], s["raw"]) if s["legal"] else (-1, b"")), (s["name"], r)
            n += s["legal"]
        for s in K.lz4_streams(body, 4096):
            r, o = D.decode(s["bytes"], s["U"] + 64, D.dictionary(4096))
            assert (r, o) == ((s["U"], s["raw"]) if s["legal"] else (-7, b"")), ("dict", s["name"], r)
            assert not s["legal"] or oracle.lz4_decompress_raw(s["bytes"], s["U"] + 64)[0] < 0      # ... and needs the dictionary
    assert n >= 3 * 18          # tails 5 .. 13, 15, 16, 270 and the six behind a long last match (tail 4 too where the body's own last match has an extension byte)
    for body in K.SNAPPY_BODIES:
        for s in K.snappy_streams(body):
            assert oracle.snappy_decompress(K.varint(s["U"]) + s["elements"], s["U"] + 64) == (s["U"], s["raw"]), s["name"]
    s = K.big_streams()
    assert oracle.lz4_decompress_raw(s["bytes"], s["U"] + 64) == (s["U"], s["raw"])
    assert oracle.snappy_decompress(K.varint(s["U"]) + s["elements"], s["U"] + 64) == (s["U"], s["raw"])
    assert max(off for _, off, _ in s["seqs"]) == 65535 and 98304 + 16 < s["U"] - 24


def _element_forms(e):
    """(sizes of the literal headers, kinds of the copy elements) of an element stream: a plain element walk"""
    hdrs, kinds, ip = set(), set(), 0
    while ip < len(e):
        tag = e[ip]; kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1; nb = max(ln - 60, 0); ip += 1
            if nb: ln = int.from_bytes(e[ip:ip + nb], "little") + 1
            hdrs.add(1 + nb); ip += nb + ln
        else:
            kinds.add(kind); ip += (0, 2, 3, 5)[kind]
    assert ip == len(e)
    return hdrs, kinds


def test_the_snappy_streams_use_every_header_form():
    for body in K.SNAPPY_BODIES:
        for s in K.snappy_streams(body):
            assert _element_forms(s["elements"]) == ({1, 2, 3}, {1, 2, 3}), s["name"]
    assert _element_forms(K.big_streams()["elements"]) == ({1, 2, 3}, {1, 2, 3})


def _walk(at, fast, b):
    """the elements of a stream, read from the input bytes only (the straight-line step checked next to the general one), or None"""
    at = M.with_fast(at, fast)
    out, ip = [], 0
    while True:
        ok, lit, mlen, off, nxt, last = at(b, ip, len(b))
        if not ok: return None
        out.append((lit, mlen, off, last or nxt == M.END))
        if last or nxt == M.END: return out
        ip = nxt


def _lz4_model(els, blob, cap):
    if cap == 0 or len(blob) == 0:                        # the kernels' prologue: the empty block into no room
        return 0 if blob == b"\x00" and cap == 0 else -7
    if els is None: return -7
    op = 0
    for lit, mlen, off, last in els:
        ok, op, fin = M.lz4_check(lit, mlen, off, last, op, cap)
        if not ok: return -7
        if fin: return op
    return -7


def _snappy_model(els, dn, cap, body_len):
    """verdict and size only (the error's name is the prologue's and the wave kernel's business)"""
    if dn > cap or dn == 0 or body_len == 0 or els is None: return -1
    op = 0
    for lit, mlen, off, last in els:
        ok, op, _ = M.snappy_check(lit, mlen, off, last, op, dn)
        if not ok: return -1
    return op if op == dn else -1


def _by_stream(cases):
    out = {}
    for c in cases: out.setdefault(c["stream"], []).append(c)
    return out


@pytest.mark.parametrize("body", K.LZ4_BODIES + ("big",))
def test_lz4_model_gives_the_oracles_verdict_and_size_on_every_case(body):
    cases = K.big_cases("lz4") if body == "big" else K.lz4_cases(body)
    for name, cs in _by_stream(cases).items():
        els = _walk(M.seq_at, M.lz4_fast_step, cs[0]["bytes"])
        for c in cs:
            assert _lz4_model(els, c["bytes"], c["cap"]) == c["result"], (name, c["cap"], c["U"], c["result"])


@pytest.mark.parametrize("body", K.SNAPPY_BODIES + ("big",))
def test_snappy_model_gives_the_oracles_verdict_and_size_on_every_case(body):
    cases = K.big_cases("snappy") if body == "big" else K.snappy_cases(body)
    for name, cs in _by_stream(cases).items():
        els = None
        for c in cs:
            blob = c["bytes"]
            hdr = next(i for i, x in enumerate(blob) if x < 0x80) + 1
            dn = sum((x & 0x7f) << (7 * i) for i, x in enumerate(blob[:hdr]))
            if els is None: els = _walk(M.snappy_at, M.snappy_fast_step, blob[hdr:])
            r = _snappy_model(els, dn, c["cap"], len(blob) - hdr)
            assert (r < 0) == (c["result"] < 0) and (r < 0 or r == c["result"]), (name, c["cap"], dn, c["U"], r, c["result"])


@pytest.mark.parametrize("body", K.LZ4_BODIES)
def test_system_liblz4_agrees_on_tails_of_5_or_more_literals(body):
    L = D.liblz4()
    if L is None or not hasattr(L, "LZ4_decompress_safe"):
        pytest.skip("no system liblz4")
    L.LZ4_decompress_safe.restype = C.c_int
    L.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    n = 0
    for c in K.lz4_cases(body):
        if c["final_lits"] < 5: continue                  # (liblz4's fast loop accepts some of those: not the reference there)
        out = C.create_string_buffer(max(c["cap"], 1))
        r = L.LZ4_decompress_safe(c["bytes"], out, len(c["bytes"]), c["cap"])
        assert (r if r >= 0 else -7, out.raw[:max(r, 0)]) == (c["result"], c["out"]), (c["stream"], c["cap"], r, c["result"])
        n += 1
    assert n > 3000


@pytest.mark.parametrize("body", K.LZ4_BODIES)
def test_the_sweep_is_not_hollow(body):
    cs = K.lz4_cases(body)
    acc = [c for c in cs if c["result"] >= 0]
    assert len(acc) >= 150 and len(cs) - len(acc) >= 3000, (len(acc), len(cs))
    assert any(c["cap"] > c["U"] and c["final_lits"] < 5 for c in acc)             # legality depends on the capacity, not on the data
    assert any(c["result"] < 0 and c["cap"] >= c["U"] for c in cs)
    assert all(c["result"] == c["U"] for c in acc)                                 # a block is never accepted short of its end
    assert max(c["cap"] for c in cs) <= 16384 and max(len(c["bytes"]) for c in cs) <= 16384 - 32      # every chunk fits all three windows


@pytest.mark.parametrize("body", K.SNAPPY_BODIES)
def test_the_snappy_sweep_is_not_hollow(body):
    cs = K.snappy_cases(body)
    acc = [c for c in cs if c["result"] >= 0]
    assert len(acc) >= 150 and len(cs) - len(acc) >= 3000, (len(acc), len(cs))
    assert {c["result"] for c in cs if c["result"] < 0} == {-11, -12}               # out_cap below the declared length / a stream that does not decode to it
    assert max(c["cap"] for c in cs) <= 16384 and max(len(c["bytes"]) for c in cs) <= 16384 - 32
