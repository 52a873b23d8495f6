"""The DEFLATE decoder held to streams zlib never writes, on the CPU: the synthesizer of tests/deflate_synth.py against zlib alone
(every case accepted with the generator's own bytes, every listed feature in three cases or more and found again by a parser of this
file's own), and the kernel's decoder compiled for the host (tests/hostsim/sim_deflate_decode.cpp) against live zlib over every
synthesized case and every stream of libdeflate and zopfli (tests/golden/golden_deflate_others.*): capacities n, n + 64, n - 1 and 0 and
each case's cuts, input misalignments 0..3, size mode, and fresh seeded single-bit flips.  No GPU."""
import collections
import ctypes as C
import os
import random
import struct
import sys

import pytest

import deflate_cases as D
import deflate_synth as S


# ---- a parser of this file's own: nothing of the decoder under test, nothing of the generator's tables --------------------------------
class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def peek(self, n):
        return (int.from_bytes(self.d[self.p >> 3:(self.p >> 3) + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def bits(self, n):
        if self.p + n > 8 * len(self.d):
            raise EOFError
        v = self.peek(n)
        self.p += n
        return v

    def sym(self, table):
        v, code = self.peek(15), 0
        for ln in range(1, 16):
            code = code << 1 | (v >> (ln - 1)) & 1
            if (ln, code) in table:
                self.p += ln
                return table[ln, code]
        raise ValueError("no code")


def _codes(lens):
    """(length, code) -> symbol, RFC 1951 3.2.2"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for bits in range(1, 16):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[l, nxt[l]] = s
            nxt[l] += 1
    return table


def _widths(lens, root):
    by = {}
    for (l, c) in _codes(lens):
        if l > root:
            by[c >> (l - root)] = max(by.get(c >> (l - root), 0), l - root)
    return set(by.values())


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _parse(raw):
    """(blocks, output or None): per block its type, the bit offset of its header, a dynamic header's fields and run-length events
    (symbol, first index, count), and the block's events ("lit", run length) / ("match", length symbol, extra, length, distance)"""
    b, out, blocks = _Bits(raw), bytearray(), []
    while True:
        blk = dict(at=b.p, final=b.bits(1), type=b.bits(2), events=[])
        blocks.append(blk)
        if blk["type"] == 0:
            b.p += -b.p % 8
            n = b.bits(16)
            assert b.bits(16) == n ^ 0xFFFF
            blk["len"] = n
            out += raw[b.p >> 3:(b.p >> 3) + n]
            b.p += 8 * n
        else:
            if blk["type"] == 1:
                lit, dist = _codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _codes([5] * 30)
            else:
                nlen, ndist, ncode = b.bits(5) + 257, b.bits(5) + 1, b.bits(4) + 4
                cl = [0] * 19
                for k in range(ncode):
                    cl[_ORDER[k]] = b.bits(3)
                ct, lens, runs = _codes(cl), [], []
                while len(lens) < nlen + ndist:
                    s = b.sym(ct)
                    if s < 16:
                        lens.append(s)
                        continue
                    n = 3 + b.bits(2) if s == 16 else 3 + b.bits(3) if s == 17 else 11 + b.bits(7)
                    runs.append((s, len(lens), n))
                    lens += [lens[-1] if s == 16 else 0] * n
                assert len(lens) == nlen + ndist
                blk.update(nlen=nlen, ndist=ndist, ncode=ncode, cl=cl, runs=runs, lens=lens, litlens=lens[:nlen], distlens=lens[nlen:])
                if lens[256] == 0:
                    return blocks, None                                       # no end-of-block code: a refusal
                lit, dist = _codes(lens[:nlen]), _codes(lens[nlen:])
            run = 0
            while True:
                s = b.sym(lit)
                if s < 256:
                    out.append(s)
                    run += 1
                    continue
                if run:
                    blk["events"].append(("lit", run))
                    run = 0
                if s == 256:
                    break
                x = b.bits(_LEXTRA[s - 257])
                n = _LBASE[s - 257] + x
                ds = b.sym(dist)
                d = _DBASE[ds] + b.bits(_DEXTRA[ds])
                assert d <= len(out)
                blk["events"].append(("match", s, x, n, d, ds))
                for _ in range(n):
                    out.append(out[-d])
        if blk["final"]:
            return blocks, bytes(out)


def _found(blocks):
    """the feature names that the parsed stream really has"""
    f = set()
    dyn = [k for k in blocks if k["type"] == 2]
    for k in dyn:
        ll, dl, nlen = k["litlens"], k["distlens"], k["nlen"]
        f |= {"lit_len_15"} if 15 in ll else set()
        f |= {"dist_len_15"} if 15 in dl else set()
        f |= {"lit_subtable_width_%d" % w for w in _widths(ll, 9)} | {"dist_subtable_width_%d" % w for w in _widths(dl, 6)}
        f |= {"all_286"} if nlen == 286 and min(ll) > 0 else set()
        f |= {"all_30"} if k["ndist"] == 30 and min(dl) > 0 else set()
        used = sum(1 for l in dl if l)
        f |= {"one_distance_code"} if used == 1 else {"no_distance_code"} if used == 0 else set()
        for s, at, n in k["runs"]:
            if at < nlen < at + n:
                f.add("run%d_crosses_alphabets" % s)
            if s == 18 and n == 138:
                f.add("run18_138")
            if s == 16 and k["lens"][at - 1] == 0:
                f.add("run16_after_zero")
        f |= {"hclen_%d" % k["ncode"]} | ({"cl_code_len_7"} if 7 in k["cl"] else set()) | ({"hlit_257"} if nlen == 257 else set()) | ({"hdist_1"} if k["ndist"] == 1 else set())
    ms = [e for k in blocks for e in k["events"] if e[0] == "match"]
    f |= {"pair_%d_%d" % (e[4], e[3]) for e in ms}
    if any(e[1] == 284 and e[2] == 31 for e in ms):
        f.add("len258_as_284_31")
    if any(e[4] == 32768 for e in ms):
        f.add("distance_32768")
    first_last = lambda sym, x, extra: {(sym, "first")} if x == 0 and extra else {(sym, "last")} if x == (1 << extra) - 1 and extra else set()
    seen = set()
    for e in ms:
        seen |= first_last(e[1], e[2], _LEXTRA[e[1] - 257]) | first_last(-e[5], e[4] - _DBASE[e[5]], _DEXTRA[e[5]])
    if all((s, w) in seen for w in ("first", "last") for s in [257 + k for k in range(8, 28)] + [-k for k in range(4, 30)]):
        f.add("max_extra_bits")
    for k in blocks:
        ev = k["events"]
        for i, e in enumerate(ev):
            if e[0] == "lit":
                nxt = ev[i + 1][0] if i + 1 < len(ev) else None
                at_start = i == 0 or ev[i - 1][0] == "match"
                if nxt == "match" and 1 <= ev[i + 1][4] <= e[1] % 64:
                    f.add("match_reads_the_literals_of_its_own_round")
                if at_start:
                    ending = "match" if nxt == "match" else "end_of_stream" if k["final"] else "end_of_block"
                    f |= {"literal_run_%d_ended_by_%s" % (e[1], ending), "literal_run_%d_ended_by_capacity" % e[1]}
        if k["type"] == 0:
            f.add("stored_%d_at_bit_%d" % (k["len"], k["at"] % 8))
    for n in (2, 3):
        if any(all(k["type"] == 0 for k in blocks[i:i + n]) for i in range(len(blocks) - n + 1)):
            f.add("stored_back_to_back_%d" % n)
    return f


def _body(c):
    s = c.stream
    return s if c.wrap == D.RAW else s[2:] if c.wrap == D.ZLIB else s[D.gzip_header_len(s):]


# ---- the generator against the reference alone -----------------------------------------------------------------------------------
def test_zlib_accepts_every_synthesized_case_with_the_generators_bytes():
    cs = S.cases()
    assert 300 <= len(cs) and sum(len(c.expected or b"") for c in cs) < 5 << 20
    for c in cs:
        r, out = D.verdict(c.wrap, c.stream, None)
        if c.expected is None:                                               # hclen_4 alone (deflate_synth's docstring)
            assert "hclen_4" in c.features and r == D.CORRUPT, (c.name, r)
            continue
        assert r == len(c.expected) and out == c.expected, (c.name, r, len(c.expected))
        assert len(c.expected) <= (70000 if c.features & {"distance_32768"} or "65535" in c.name else 65536), c.name
    raw = [c for c in cs if c.wrap == D.RAW]
    assert len(raw) + 3 <= len(cs) and 0.2 < sum(1 for c in cs if c.wrap == D.ZLIB) / len(raw) < 0.45
    assert sum(1 for c in cs if c.wrap == D.ZLIB) + 3 == sum(1 for c in cs if c.wrap == D.GZIP)
    assert {c.features & {"codes", "headers", "matches", "literal_runs", "stored", "blocks"} for c in cs} == {frozenset([f]) for f in ("codes", "headers", "matches", "literal_runs", "stored", "blocks")}


def test_every_feature_is_in_three_cases_and_really_there():
    """counted from the generator's own `features`; each claim checked on the stream itself by this file's parser"""
    cs = S.cases()
    count = collections.Counter(f for c in cs for f in c.features)
    for f in S.LISTED:
        assert count[f] >= 3, (f, count[f])
    want = (["pair_%d_%d" % (d, n) for d in S.GRID_DISTANCES for n in S.GRID_LENGTHS]
            + ["literal_run_%d_ended_by_%s" % (r, e) for r in S.RUNS for e in ("match", "end_of_block", "end_of_stream", "capacity")]
            + ["stored_%d_at_bit_%d" % (n, b) for n in S.STORED_LENGTHS for b in range(8)] + ["stored_back_to_back_2", "stored_back_to_back_3"]
            + ["blocks_40", "empty_fixed", "empty_dynamic", "final_empty_stored", "zlib_cinfo_0", "zlib_cinfo_7", "gzip_fextra_none", "gzip_fname_300", "gzip_fcomment_300",
               "gzip_fhcrc_on", "gzip_fhcrc_off"] + ["gzip_fextra_%d" % n for n in S.FEXTRA])
    for f in want:
        assert count[f] >= 1, f
    for d in S.GRID_DISTANCES:                                               # the grid in fixed AND in dynamic blocks
        for kind in ("_fixed", "_dynamic"):
            assert any(c.name.endswith(kind) and "pair_%d_258" % d in c.features for c in cs), (d, kind)
    for c in cs:
        blocks, out = _parse(_body(c))
        assert out == c.expected, c.name
        found = _found(blocks)
        claimed = {f for f in c.features if f in S.LISTED or f.startswith(("pair_", "literal_run_", "stored_", "hclen_"))}
        assert claimed <= found, (c.name, sorted(claimed - found))
        if c.wrap == D.ZLIB:
            assert "zlib_cinfo_%d" % (c.stream[0] >> 4) in c.features and (c.stream[0] >> 4 or max([e[4] for k in blocks for e in k["events"] if e[0] == "match"] or [0]) <= 256)
        if c.wrap == D.GZIP:
            flg, s = c.stream[3], c.stream
            assert ("gzip_fextra_%d" % (s[10] | s[11] << 8) if flg & 4 else "gzip_fextra_none") in c.features
            assert ("gzip_fname_300" in c.features) == bool(flg & 8) and ("gzip_fcomment_300" in c.features) == bool(flg & 16) and ("gzip_fhcrc_on" in c.features) == bool(flg & 2)
    counts = collections.Counter(len(_parse(_body(c))[0]) for c in cs if "blocks" in c.features)
    assert counts[1] >= 3 and counts[2] >= 9 and counts[40] >= 3
    orders = {tuple(k["type"] for k in _parse(_body(c))[0]) for c in cs if "blocks" in c.features}
    assert {(a, b) for a in range(3) for b in range(3)} | {(a,) for a in range(3)} <= orders


def test_other_encoders_fixtures_cover_their_matrix_and_are_what_zlib_says_today():
    vs, ms = D.others(), D.other_mutations()
    pay = D.payloads()
    enc = {"libdeflate1", "libdeflate6", "libdeflate9", "libdeflate12", "zopfli3"}
    for p in ("text300", "text4k", "corpus64k", "zeros64k", "dist32768"):
        assert {v["encoder"] for v in vs if v["payload"] == p and v["wrap"] == D.RAW} == enc, p
    for p in ("text4k", "corpus64k"):
        assert {(v["encoder"], v["wrap"]) for v in vs if v["payload"] == p} == {(e, w) for e in enc for w in D.WRAPS}
    assert {v["encoder"] for v in vs if v["payload"] == "random64k"} >= {"libdeflate1", "zopfli3"} and sum(1 for v in vs if v["n"] == 200000) >= 2
    assert all(D.sha(pay[v["payload"]]) == v["sha256"] for v in vs if v["payload"] in pay)
    ok = sum(1 for m in ms if m["result"] >= 0)
    assert len(ms) == 200 and ok >= 20 and len(ms) - ok >= 20 and len({m["base"] for m in ms}) == 4
    for c in vs + ms:
        r, out = D.verdict(c["wrap"], c["bytes"], c["cap"])
        assert r == c["result"] and (r < 0 or (len(out) == c["n"] and D.sha(out) == c["sha256"])), c["name"]
    # what zlib's own streams never hold: distances beyond 32 506 (this file's parser says so; 32 767 and 32 768 are the synthesizer's)
    far = [v["name"] for v in vs if v["wrap"] == D.RAW and v["payload"] in ("dist32768", "corpus64k", "corpus200k")
           and any(e[0] == "match" and e[4] > 32506 for k in _parse(v["bytes"])[0] for e in k["events"])]
    assert len(far) == 14, far
    meta = D._load_others()[0]
    assert set(meta["libraries"]) == {"libdeflate", "zopfli"} and all(len(v["sha256"]) == 64 and v["path"] for v in meta["libraries"].values())


def test_other_encoders_minted_live_equal_the_file():
    """where both libraries load (they are not part of the project: skipped elsewhere) and are the recorded files"""
    sys.path.insert(0, D.GOLDEN)
    try:
        import make_golden_deflate_others as M
    finally:
        sys.path.remove(D.GOLDEN)
    try:
        compress, libs = M.load()
    except (OSError, AttributeError) as ex:
        pytest.skip("libdeflate / zopfli do not load here: %s" % ex)
    meta, blob = D._load_others()
    if {k: v["sha256"] for k, v in libs.items()} != {k: v["sha256"] for k, v in meta["libraries"].items()}:
        pytest.skip("other builds of libdeflate / zopfli than the ones that minted the file")
    got_blob, rows, muts = M.mint(compress)
    assert got_blob == blob and rows == meta["valid"] and muts == meta["mutations"]


# ---- the host build against live zlib -------------------------------------------------------------------------------------------------
def _sim(wrap, s, cap, mis, size=False):
    L = D.sim_lib()
    buf = C.create_string_buffer(len(s) + 32)
    at = C.addressof(buf) + (-C.addressof(buf)) % 16 + mis
    C.memmove(at, s, len(s))
    out = C.create_string_buffer(max(cap, 1))
    r = L.sim_deflate_decode(wrap, 1 if size else 0, at, len(s), out, cap)
    return r, (out.raw[:r] if r > 0 and not size else b"")


def _hold_to_zlib(name, wrap, s, caps):
    """every capacity x misalignments 0..3 and size mode; returns the number of decodes"""
    runs = 0
    for cap in caps:
        want = D.verdict(wrap, s, cap)
        for mis in range(4):
            got = _sim(wrap, s, cap, mis)
            assert got[0] == want[0] and (got[0] < 0 or got[1] == want[1]), (name, cap, mis, got[0], want[0])
            runs += 1
    want = D.size_verdict(wrap, s)
    for mis in range(4):
        assert _sim(wrap, s, 0, mis, size=True)[0] == want, (name, "size", mis, want)
    return runs + 4


def _caps(n, cuts=()):
    return sorted({n, n + 64, max(n - 1, 0), 0} | set(cuts)) if n >= 0 else [300, 0]


def _left_out(names):
    skip = [n for n in names if n in D.DIVERGES_FROM_ZLIB]
    total = len(D.valid()) + len(D.mutations()) + len(D.hand()) + len(S.cases()) + len(D.others()) + len(D.other_mutations())
    assert len(D.DIVERGES_FROM_ZLIB) <= 0.02 * total and len(D.DIVERGES_FROM_ZLIB) <= 0.02 * (len(D.valid()) + len(D.mutations()) + len(D.hand()))
    return set(skip)


@pytest.mark.parametrize("family", ("codes", "headers", "matches", "literal_runs", "stored", "blocks"))
def test_host_build_equals_zlib_on_every_synthesized_case(family):
    """capacities n, n + 64, n - 1, 0 and the case's cuts (a literal run cut at 62..65 literals, a stored block at its edges: the
    one-byte-over rule of deflate_wave_walk), misalignments 0..3, size mode"""
    cs = [c for c in S.cases() if family in c.features]
    skip = _left_out([c.name for c in cs])
    runs = 0
    for c in cs:
        if c.name in skip:
            continue
        n = len(c.expected) if c.expected is not None else -1
        if family == "literal_runs":
            assert c.cuts or c.name.startswith("literal_run_1_"), c.name
        if family == "stored":
            assert len(c.cuts) >= 3 or "stored_0_" in c.name, c.name
        runs += _hold_to_zlib(c.name, c.wrap, c.stream, _caps(n, c.cuts))
    assert runs >= 12 * (len(cs) - len(skip))


def test_host_build_equals_zlib_on_the_other_encoders_streams():
    cs = D.others() + D.other_mutations()
    skip = _left_out([c["name"] for c in cs])
    for c in cs:
        if c["name"] in skip:
            continue
        r, out = _sim(c["wrap"], c["bytes"], c["cap"], 0)
        assert r == c["result"] and (r < 0 or D.sha(out) == c["sha256"]), c["name"]
        _hold_to_zlib(c["name"], c["wrap"], c["bytes"], _caps(c["result"]) if c["result"] >= 0 else [c["cap"], 64, 0])


def test_fresh_single_bit_flips_of_synthesized_cases_against_live_zlib():
    """1 800 seeded flips, two in three within the first 400 bytes (the headers and the code lengths); both verdicts occur often"""
    rng = random.Random(99)
    pool = [c for c in S.cases() if c.expected is not None and len(c.stream) < 40000]
    seen = collections.Counter()
    for k in range(1800):
        c = pool[rng.randrange(len(pool))]
        span = min(len(c.stream), 400) if k % 3 else len(c.stream)
        s = D.flip(c.stream, rng.randrange(8 * span))
        cap = len(c.expected) + (0, 300, -1, 64)[k % 4]
        if cap < 0:
            cap = 0
        want = D.verdict(c.wrap, s, cap)
        got = _sim(c.wrap, s, cap, k % 4)
        assert got[0] == want[0] and (got[0] < 0 or got[1] == want[1]), (c.name, k, cap, got[0], want[0])
        seen[want[0] >= 0] += 1
    print(dict(seen))
    assert seen[True] >= 100 and seen[False] >= 100


def test_the_cases_file_of_the_stand_alone_program(tmp_path):
    """deflate_synth.write_cases_file: the header and the first record are what tests/hostsim/sim_deflate_decode.cpp's main reads"""
    path = os.path.join(str(tmp_path), "cases.bin")
    keep = S.cases()
    n = S.write_cases_file(path, [(o["name"], o["wrap"], o["bytes"]) for o in D.others()[:2]], only=keep[:7])
    with open(path, "rb") as f:
        blob = f.read()
    assert struct.unpack_from("<I", blob)[0] == n >= 9 * 5
    wrap, size, ln, cap, mis, want = struct.unpack_from("<5Iq", blob, 4)
    c = keep[0]
    assert (wrap, size, ln, cap, mis, want) == (c.wrap, 0, len(c.stream), len(c.expected), 0, len(c.expected))
    assert blob[32:32 + ln] == c.stream and blob[32 + ln:32 + ln + want] == c.expected
