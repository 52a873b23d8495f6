"""What tests/test_scratch_streams_gpu.py rests on, without a GPU: for every pairing of tests/scratch_streams_cases.py the expected
results and bytes agree with the references and with the case modules' recorded verdicts, X runs at least eight slices over the three
slots its shrunken budget leaves (from the slot sizes include/cramjam_hip_debug.h states), malformed inputs sit between the good ones of
every call, and no input is one that makes the CALL fail.  Without this the GPU test could quietly compare nothing with nothing."""
import gzip
import os
import re
import struct
import zlib

import pytest

import oracle
import scratch_streams_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("P1", "P1k", "P2", "P3", "P4", "P5", "P6", "P7", "P8")
BUDGETED = {"P5": ["cj_debug_zstd_slot_budget"], "P6": ["cj_debug_bgzf_slot_budget", "cj_debug_deflate_slot_budget"],
            "P7": ["cj_debug_zstd_enc_slot_budget"], "P8": ["cj_debug_dict_stage_budget"]}


@pytest.fixture(scope="module")
def ps():
    return S.pairings()


def test_the_slot_sizes_are_the_debug_headers():
    with open(os.path.join(ROOT, "include", "cramjam_hip_debug.h")) as f:
        text = re.sub(r"\s*\n\s*\*?\s*", " ", f.read())
    assert "one slot of 128 KiB + 32 per stream in flight" in text and S.ZSTD_SLOT == 128 * 1024 + 32
    assert "one slot of 320.25 KiB per frame" in text and S.ZSTD_ENC_SLOT == int(320.25 * 1024)
    assert "one slot of 256.25 KiB per stream in flight" in text and S.DEFLATE_SLOT == int(256.25 * 1024)
    assert "one slot of 65 312 bytes per member" in text and S.BGZF_SLOT == 65312
    # the dictionary encoder's slot is `dictionary tail | chunk` (cj_debug_dict_stage_budget): the 4 096 bytes that count, a chunk of at most 64 KiB
    assert S.DICT_SLOT >= S.DICT_LEN + 65536 and S.DICT_SLOT % 256 == 0


def test_every_pairing_of_the_table_is_there_with_its_budget(ps):
    assert tuple(ps) == NAMES
    for name, p in ps.items():
        assert [b[0] for b in p.budgets] == BUDGETED.get(name, []), name
        for fn, nbytes in p.budgets:
            slot = {"cj_debug_zstd_slot_budget": S.ZSTD_SLOT, "cj_debug_bgzf_slot_budget": S.BGZF_SLOT, "cj_debug_deflate_slot_budget": S.DEFLATE_SLOT,
                    "cj_debug_zstd_enc_slot_budget": S.ZSTD_ENC_SLOT, "cj_debug_dict_stage_budget": S.DICT_SLOT}[fn]
            assert nbytes // slot == (S.BGZF_SLOTS if "bgzf" in fn else S.SLOTS) and nbytes % slot == 0, (name, fn)
        assert p.x.chunks != p.y.chunks, name                         # other data on the other stream
    assert ps["P1"].x.flags == 0 and ps["P1"].x.n <= 16384            # CJ_FUSED_MAX_CHUNKS: the one-kernel path
    assert ps["P1k"].x.flags and ps["P1k"].y.flags
    assert sum(1 for p in ps.values() if p.x.entry != p.y.entry) >= len(ps) // 2
    assert ps["P1"].host_mode and ps["P5"].host_mode


def test_x_runs_at_least_eight_slices_over_three_slots(ps):
    for name in BUDGETED:
        p = ps[name]
        print(name, p.scratch, "slices of X, Y:", p.slices)
        assert p.slices[0] >= S.MIN_SLICES and p.slices[1] >= 2, (name, p.slices)
    # the arithmetic behind them
    assert ps["P5"].slices == (-(-S.blosc_zstd_rows(ps["P5"].x) // 3), -(-ps["P5"].y.n // 3))
    assert S.blosc_zstd_rows(ps["P5"].x) >= 24
    x = ps["P6"].x
    assert len([c for c in x.chunks]) >= 8 and all(3 <= -(-len(c) // 65280) <= 5 for c in x.chunks)
    assert ps["P6"].slices[0] == -(-S.bgzf_members(x) // 2) >= 8      # one DEFLATE slice per BGZF turn of two members
    assert ps["P7"].slices[0] == -(-ps["P7"].x.n // 3) and ps["P8"].slices[0] == -(-ps["P8"].x.n // 3)
    # `scratch` and `fb` have no budget: both calls lay their tables out from the first byte, more than one unit of work each
    for name in ("P1", "P1k", "P2", "P3", "P4"):
        assert ps[name].slices is None and ps[name].x.n >= 8 and ps[name].y.n >= 8, name


def test_malformed_inputs_sit_between_good_ones_and_no_call_fails(ps):
    for name, p in ps.items():
        for c in (p.x, p.y):
            good = [w.good for w in c.want]
            assert 1 <= good.count(False) < good.count(True) or c.entry == "bgzf_decompress_many_device", (name, c.label)
            assert good.count(False) >= 1 and good.count(True) >= 8, (name, c.label)
            first, last = good.index(False), len(good) - 1 - good[::-1].index(False)
            assert any(good[:first]) and (any(good[last:]) or any(good[first:last])), (name, c.label)
            # what makes a CALL fail: no chunks, an address range beyond the buffers, more than 2^32 - 16 block rows; a chunk above a limit only fails itself
            size, off, ln, ooff, total = c.layout()
            assert c.n > 0 and size < (64 << 20) and total < (64 << 20), (name, c.label, size, total)
            assert all(o + n <= size for o, n in zip(off, ln)) and all(o + cap + S.G <= total for o, cap in zip(ooff, c.caps))
            assert all(len(x) <= 0x7E000000 and cap <= 0x7E000000 for x, cap in zip(c.chunks, c.caps))
            if c.dictionary is not None:
                assert sum(1 for x in c.chunks if len(x) > 65536) == 1 and len(c.dictionary) == S.DICT_LEN


def _lz4_and_snappy(c, decode):
    for s, cap, w in zip(c.chunks, c.caps, c.want):
        r, o = decode(s, cap)
        if w.good:
            assert (r, o) == (len(w.data), w.data), c.label
        else:
            assert r < 0 and w.code in (S.LZ4_CORRUPT, r), (c.label, r, w.code)


def test_block_and_frame_expectations_are_the_oracles(ps):
    import base64
    _lz4_and_snappy(ps["P1"].x, oracle.lz4_decompress_raw)
    _lz4_and_snappy(ps["P4"].y, oracle.lz4_decompress_raw)
    _lz4_and_snappy(ps["P1"].y, oracle.snappy_decompress)
    assert ps["P1k"].x.chunks == ps["P1"].x.chunks and [(w.data, w.code) for w in ps["P1k"].x.want] == [(w.data, w.code) for w in ps["P1"].x.want]
    # ... and the malformed blocks carry the verdict recorded with them
    rec = {base64.b64decode(m["data"]): m["ret"] for m in S._golden()["malformed_lz4"]}
    bad = [(s, w) for s, w in zip(ps["P1"].x.chunks, ps["P1"].x.want) if s in rec and not w.good]
    assert len(bad) >= 5 and all(rec[s] < 0 for s, _w in bad)
    rec = {base64.b64decode(m["data"]): m["ret"] for m in S._golden()["malformed_snappy"]}
    bad = [(s, w) for s, w in zip(ps["P1"].y.chunks, ps["P1"].y.want) if s in rec and not w.good]
    assert len(bad) >= 5 and all(rec[s] < 0 for s, _w in bad)
    x = ps["P2"].x
    assert x is ps["P4"].x
    for s, cap, w in zip(x.chunks, x.caps, x.want):
        r, o = oracle.lz4_frame_decompress(s, cap)
        assert (r < 0) if w.negative else (r, o) == (len(w.data), w.data)
    y = ps["P2"].y
    for raw, cap, w in zip(y.chunks, y.caps, y.want):
        if w.good:                                            # the reader that will judge the GPU's streams reads the oracle's own, and no other buffer's
            s = oracle.snappy_frame_compress(raw)[1]
            assert w.verify(s) and not w.verify(s[:-1]) and not w.verify(oracle.snappy_frame_compress(raw[:-1] + b"\0")[1]) and len(s) <= cap
        else:
            assert cap < 18                                   # not even the stream identifier and a chunk header fit


def test_blosc_and_bgzf_expectations_are_the_models_and_the_recorded_verdicts(ps):
    import bgzf_model as B
    import blosc_cases as K
    import blosc_model as M
    x = ps["P3"].x
    by = {v["bytes"]: v for v in K.valid()}
    bad = {m["bytes"]: m for m in K.malformed()}
    for s, cap, w in zip(x.chunks, x.caps, x.want):
        cls, out = M.verdict(s, cap)
        if w.good:
            v = by[s]
            assert v["recipe"]["filter"] == 1 and v["recipe"]["cname"] in ("lz4", "lz4hc") and cls == "ok" and (len(out), S.sha(out)) == (w.size, w.digest) == (v["nbytes"], v["sha256"])
        else:
            assert cls == bad[s]["verdict"] != "ok" and w.code == M.CODE[cls]
    y = ps["P3"].y
    streams = {s: k for k, (_f, s) in B.cases().items()}
    n_ok = 0
    for s, cap, w in zip(y.chunks, y.caps, y.want):
        fam = B.cases()[streams[s]][0]
        assert w.good == fam.startswith("ok"), streams[s]
        if w.good:
            assert gzip.decompress(s) == w.data and cap == len(w.data)
            n_ok += 1
        else:
            assert w.code < 0 and B.decode(s, cap)[0] == w.code
            if w.code not in (B.EOF, B.HEADER):               # the members' heads are sound: zlib is the judge of what is inside them
                with pytest.raises((zlib.error, OSError, EOFError)):
                    gzip.decompress(s)
    assert n_ok >= 30


def test_zstandard_expectations_are_the_recorded_verdicts_and_libzstds(ps):
    import blosc_model as M
    import blosc_zcodec_model as Z
    import zstd_cases as ZC
    y = ps["P5"].y
    by = {c.stream: c for c in ZC.load_cases()}
    for s, cap, w in zip(y.chunks, y.caps, y.want):
        c = by[s]
        assert cap == c.cap and ((w.size, w.digest) == (c.verdicts[0], c.sha) if c.accepted else w.code == c.verdicts[0] < 0)
        if c.name not in ZC.DIVERGES_FROM_ZSTD:
            r, o = ZC.zstd_verdict(s, cap)
            assert r == c.verdicts[0] and (r < 0 or ZC.sha(o) == c.sha), c.name
    x = ps["P5"].x
    assert x.kw == {"zstd": True}
    rec = {(v["bytes"], v["nbytes"]): ("ok", v["nbytes"], v["sha256"]) for v in Z.valid()}
    rec.update({(m["bytes"], m["cap"]): (m["verdict"], m["cap"], None) for m in Z.malformed() if m["verdict"] != "ok"})
    for s, cap, w in zip(x.chunks, x.caps, x.want):
        cls, rcap, digest = rec[(s, cap)]
        got, out = Z.verdict(s, cap)
        assert got == cls and cap == rcap, (got, cls)
        if w.good:
            assert Z.fmt_of(s) == Z.FORMAT_ZSTD and S.sha(out) == digest == w.digest and len(out) == w.size
        else:
            assert w.code == M.CODE[cls]


def _bgzf_by_the_model(buf):
    """the stream the BGZF encoder is to write: per piece of 65 280 bytes the marker's head with BSIZE, the DEFLATE model's raw bytes, CRC32, ISIZE"""
    import bgzf_model as B
    import deflate_enc_cases as E
    out = b""
    for at in range(0, len(buf), B.PIECE):
        piece = buf[at:at + B.PIECE]
        body = E.model(piece, E.RAW)[1]
        out += B.MARKER[:16] + struct.pack("<H", 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(piece), len(piece))
    return out + B.MARKER


def test_encoder_expectations_are_the_models_and_read_back(ps):
    import bgzf_model as B
    import deflate_enc_cases as E
    import zstd_cases as ZC
    import zstd_enc_cases as ZE
    x = ps["P6"].x
    for buf, cap, w in zip(x.chunks[:3] + x.chunks[-2:], x.caps[:3] + x.caps[-2:], x.want[:3] + x.want[-2:]):
        if w.good:
            s = _bgzf_by_the_model(buf)
            assert w.verify(s) and len(s) <= cap == B.compress_bound(len(buf))
            assert not w.verify(B.stream([buf[i:i + B.PIECE] for i in range(0, len(buf), B.PIECE)]))      # zlib's members: read back, but not the model's
            assert not w.verify(s[:-len(B.MARKER)])
        else:
            assert w.code == B.OUT_TOO_SMALL and cap < 28
    y = ps["P6"].y
    assert y.kw == {"wrapper": "zlib"}
    for data, cap, w in zip(y.chunks, y.caps, y.want):
        r, s = E.model(data, E.ZLIB, cap)[:2]
        if w.good:
            assert s == w.data and zlib.decompress(s) == data and cap == E.bound(len(data), E.ZLIB)
        else:
            assert r == w.code == S.OUT_TOO_SMALL and E.model(data, E.ZLIB, cap + 1)[0] == cap + 1
    for c, flags in ((ps["P7"].x, 0), (ps["P7"].y, 1)):
        assert c.kw == {"checksum": bool(flags)}
        for data, cap, w in zip(c.chunks, c.caps, c.want):
            r, s = ZE.model(data, flags, cap)[:2]
            if w.good:
                assert s == w.data and ZC.zstd_verdict(s, len(data)) == (len(data), data) and cap == ZE.bound(len(data), flags)
                assert (s[4] >> 2) & 1 == flags
            else:
                assert r == w.code == S.OUT_TOO_SMALL and ZE.model(data, flags, cap + 1)[0] == cap + 1
    assert not set(ps["P7"].x.chunks) & set(ps["P7"].y.chunks)


def test_dictionary_expectations_are_the_linked_model_and_decode(ps):
    import lz4_dict_model as D
    assert not set(ps["P8"].x.chunks) & set(ps["P8"].y.chunks)
    for c in (ps["P8"].x, ps["P8"].y):
        assert c.dictionary == D.dictionary(S.DICT_LEN) and c.kw == {"store_size": False}
        for raw, cap, w in zip(c.chunks, c.caps, c.want):
            if w.good:
                assert D.decode(w.data, len(raw), c.dictionary) == (len(raw), raw) and len(w.data) <= cap
                assert D.decode(w.data, len(raw), b"")[0] < 0 or D.decode(w.data, len(raw), b"")[1] != raw or len(raw) < 64      # (it does lean on the dictionary)
            else:
                assert len(raw) == 65537 and w.code == S.INPUT_TOO_LARGE


def test_a_want_finds_what_is_wrong():
    import numpy as np
    w = S.Want(data=b"abcdef")
    assert w.problem(6, b"abcdefzz") is None and w.problem(5, b"abcdef") and w.problem(6, b"abcdeX") and w.problem(-7, b"")
    assert S.Want(code=-7).problem(-7, b"") is None and S.Want(code=-7).problem(-6, b"") and S.Want(negative=True).problem(0, b"")
    assert S.Want(size=3, digest=S.sha(b"xyz")).problem(3, b"xyz!") is None and S.Want(size=3, digest=S.sha(b"xyz")).problem(3, b"xyy")
    c = S.Call("t", "e", [b"1", b"2"], [8, 4], [w, S.Want(code=-7)])
    size, off, ln, ooff, total = c.layout()
    out = np.full(total, S.FILL, np.uint8)
    out[ooff[0]:ooff[0] + 6] = np.frombuffer(b"abcdef", np.uint8)
    assert c.problems([6, -7], out, ooff) == []
    out[ooff[1] + 1] = 0                                              # inside a refused chunk's slot: its own business
    assert c.problems([6, -7], out, ooff) == []
    out[ooff[1] + 4] = 0                                              # its guard
    assert [i for i, _ in c.problems([6, -7], out, ooff)] == [-1]
    out[ooff[1] + 4] = S.FILL
    out[ooff[0] + 6] = 0                                              # behind a good chunk's result, inside its slot
    assert [i for i, _ in c.problems([6, -7], out, ooff)] == [-1]
