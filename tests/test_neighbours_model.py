"""The neighbour sweep on the CPU (tests/neighbour_cases.py): the host builds of the wave decoders with the stand-in's
DEVICE-LOAD mode on — the register window reads what InWindow::load_row (cramjam_amd/csrc/cj_common.hpp) loads: the memory's own
bytes inside every dword that starts below the stream's end, the up to 3 bytes in front of a misaligned stream included, and 0 behind —
over every decoder case under all four rings, each called in place inside the packed blob, as the device is; the same cases as one
stand-alone sanitizer program per sim, whose every stream is a heap block of exactly the dwords it touches; the BloscLZ, Zlib and Zstd
streams of the Blosc chunks in place inside their chunks; that the inputs bite (with
in_len overstated by 3 the verdict does depend on the ring; a quarter of the cases and more have a straddling dword); that the
encoder inputs' `own` ring continues their period and that the encoder models' streams decode to the inputs.  No GPU."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import zlib

import pytest

import deflate_cases as DF
import neighbour_cases as NC
from hostsim_build import build_sim

SIM_BOUNDS = -9999
sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()


# ---- the stand-in's second mode ------------------------------------------------------------------------------------------------------------
def test_device_load_mode_of_the_register_window(tmp_path):
    """tests/hostsim/sim_standins.cpp, op 22: a stream of n bytes that begins `mis` bytes behind the dword boundary at arena byte 64
    (arena byte i = i).  Real bytes inside any dword that starts below iend = mis + n — below the stream's first byte and behind its
    last one alike —, 0 in every dword behind; n = 0 at mis = 0 loads nothing; the default mode is untouched by a call in this one."""
    L = C.CDLL(build_sim("sim_standins.cpp", str(tmp_path / "libsim_standins.so")))
    L.standin.restype = C.c_longlong
    L.standin.argtypes = [C.c_int, C.c_long, C.c_long, C.c_long]
    arena = bytes(range(256))

    def want(mis, n, pos):
        iend = mis + n
        return int.from_bytes(bytes(arena[64 + p] if (p & ~3) < iend else 0 for p in range(pos, pos + 4)), "little")
    for mis in range(4):
        for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, 40):                # iend on (mis + n) % 4 == 0 and off a dword boundary
            for pos in range(0, mis + n + 9):
                assert L.standin(22, mis, n, pos) == want(mis, n, pos), (mis, n, pos)
    assert L.standin(22, 0, 0, 0) == 0 and L.standin(22, 0, 4, 4) == 0                      # nothing behind a boundary that is the end
    assert L.standin(22, 3, 0, 0) == int.from_bytes(arena[64:68], "little")                 # n = 0 behind 3 bytes: dword 0 starts below iend
    assert L.standin(22, 1, 2, 0) == int.from_bytes(arena[64:68], "little")                 # one byte in front, one behind: both the neighbours'
    assert L.standin(22, 0, 5, 4) == int.from_bytes(arena[68:72], "little") and L.standin(22, 0, 5, 8) == 0
    assert L.standin(22, 0, 40, 508) == SIM_BOUNDS                                          # the window's precondition holds in both modes
    assert L.standin(16, 64, 64 + 38, 0) == int.from_bytes(arena[102:104] + b"\xee\xee", "little")      # the default is still 0xEE


# ---- the sims, device-load mode on ---------------------------------------------------------------------------------------------------------
class Blob:
    """a layout's blob at a 16-byte boundary of host memory: chunk i lies at .at(i), its neighbours around it"""

    def __init__(self, blob, off):
        self.buf = (C.c_ubyte * (len(blob) + 16))()
        self.base = C.addressof(self.buf) + (-C.addressof(self.buf)) % 16
        C.memmove(self.base, blob.tobytes(), len(blob))
        self.off = [int(o) for o in off]

    def at(self, i):
        return self.base + self.off[i]


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    """every sim with the device-load mode on (and off again behind the module: tests/deflate_cases.py shares its library)"""
    import test_lz4_dict_model as TD
    d = tmp_path_factory.mktemp("neighbours")
    import test_input_sweep_model as TI
    S = {"deflate": DF.sim_lib(), "lz4_dict": TD.sim_lib(), "snappy": TI.snappy_sim_lib()}      # (lz4_dict: sim_lz4_wave.cpp, both entries)
    for name in ("zstd", "blosclz"):
        S[name] = C.CDLL(build_sim("sim_%s_decode.cpp" % name, str(d / ("libsim_%s.so" % name))))
    S["zstd"].sim_zstd_decode.restype = C.c_longlong
    S["zstd"].sim_zstd_decode.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    S["blosclz"].sim_blosclz_decode.restype = C.c_longlong
    S["blosclz"].sim_blosclz_decode.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    S["bgzf"] = C.CDLL(build_sim("sim_bgzf_grammar.cpp", str(d / "libsim_bgzf.so")))
    S["bgzf"].sim_bgzf_walk.restype = C.c_longlong
    S["bgzf"].sim_bgzf_walk.argtypes = [C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    wave = [S[k] for k in ("deflate", "lz4_dict", "snappy", "zstd", "blosclz")]
    for L in wave:
        L.sim_set_device_loads(1)
    yield S
    for L in wave:
        L.sim_set_device_loads(0)


def _ring_block(B, i, n):
    """the dwords chunk i touches, as the sanitizer programs' blocks hold them: (offset mod 4) bytes in front, the stream, up to 3 behind"""
    front = B.off[i] & 3
    return C.string_at(B.at(i) - front, (front + n + 3) & ~3)


def _sanitized(tmp_path, source, recs):
    exe = build_sim(source, str(tmp_path / "sim_main"), main=True, sanitize=True)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, path, "device"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(recs) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def _sweep(key, cases, call, record, rings=NC.RINGS):
    """every case under every ring, in place; call(ptr, n, cap, out) -> result.  The reference's result and bytes (sha256 where the
    case records one); returns the sanitizer program's records, made by record(case, offset mod 16, block, expected bytes)"""
    recs, straddle, total = [], 0, 0
    for ring in rings:
        blob, off, _, _ = NC.case_layout(key, cases, ring)
        B = Blob(blob, off)
        for i, c in enumerate(cases):
            n, cap = len(c["bytes"]), c["cap"]
            out = (C.c_ubyte * max(cap, 1))()
            r = call(B.at(i), n, cap, out)
            assert r != SIM_BOUNDS and r == c["result"], (key, ring, c["base"], c["k"], cap, B.off[i] % 16, r, c["result"])
            got = bytes(out[:r]) if r > 0 and not c.get("sized") else b""       # (a size query writes no bytes)
            if got:
                assert (got == c["out"]) if c["out"] is not None else (sha(got) == c["sha"]), (key, ring, c["base"], c["k"], cap)
            recs.append(record(c, B.off[i] % 16, _ring_block(B, i, n), got))
            straddle += (B.off[i] + n) % 4 != 0
            total += 1
        assert C.string_at(B.base, len(blob)) == blob.tobytes(), (key, ring)               # no sim writes its input
        assert not NC.alignment_coverage(cases, off), (key, ring, NC.alignment_coverage(cases, off))
    assert 4 * straddle >= total, (key, straddle, total)                                   # a quarter and more have a straddling dword
    return recs


@pytest.mark.parametrize("wrap", DF.WRAPS)
def test_deflate_decoder_and_size_query(sims, tmp_path, wrap):
    L = sims["deflate"]
    cases = NC.deflate_cases(wrap)
    rec = lambda size: (lambda c, mis, block, exp: struct.pack("<5Iq", wrap, size, len(c["bytes"]), c["cap"], mis & 3, c["result"]) + block + exp)
    recs = _sweep(("deflate", wrap), cases, lambda p, n, cap, out: L.sim_deflate_decode(wrap, 0, p, n, out, cap), rec(0))
    recs += _sweep(("deflate-size", wrap), NC.deflate_size_cases(wrap), lambda p, n, cap, out: L.sim_deflate_decode(wrap, 1, p, n, None, 0), rec(1))
    _sanitized(tmp_path, "sim_deflate_decode.cpp", recs)


def test_zstd_decoder(sims, tmp_path):
    L = sims["zstd"]
    rec = lambda c, mis, block, exp: struct.pack("<4Iq", 0, len(c["bytes"]), c["cap"], mis & 3, c["result"]) + block + exp
    _sanitized(tmp_path, "sim_zstd_decode.cpp", _sweep("zstd", NC.zstd_cases(), lambda p, n, cap, out: L.sim_zstd_decode(0, p, n, out, cap), rec))


def test_golden_neighbours_are_what_libzstd_says_today():
    import zstd_cases as Z
    try:
        Z.libzstd()
    except OSError:
        pytest.skip("libzstd is not on this machine")
    doc = NC.mint_zstd()
    doc.pop("libzstd")
    assert doc == {k: v for k, v in NC.zstd_doc().items() if k != "libzstd"}
    assert os.path.getsize(NC.GOLDEN_JSON) < 1 << 20


def test_lz4_dictionary_decoder(sims, tmp_path):
    import lz4_dict_model as D
    L = sims["lz4_dict"]
    d = D.dictionary(NC.DICT_LEN)
    dbuf = (C.c_ubyte * (len(d) + 32))()
    dptr = C.addressof(dbuf) + (-C.addressof(dbuf)) % 16 + 3
    C.memmove(dptr, d, len(d))
    rec = lambda c, mis, block, exp: struct.pack("<6Iq", len(c["bytes"]), c["cap"], len(d), mis & 3, 3, 0, c["result"]) + block + d + exp
    _sanitized(tmp_path, "sim_lz4_wave.cpp", _sweep("lz4_dict", NC.lz4_dict_cases(), lambda p, n, cap, out: L.sim_lz4_dict_decode(p, n, out, cap, dptr, len(d)), rec))


def test_plain_lz4_and_snappy_block_decoders_with_ff_in_front(sims, tmp_path):
    """the block cases of the GPU's test_block_decoders_with_ff_in_front (the `own` cuts of the input sweep's family A, body a: 48 bytes
    of 0xFF in front, the stream's continuation behind) through lz4_wave_decode<false> and snappy_wave_decode, in place and as the
    sanitizer programs"""
    L, Ls = sims["lz4_dict"], sims["snappy"]
    rec = lambda c, mis, block, exp: struct.pack("<6Iq", len(c["bytes"]), c["cap"], 0, mis & 3, 0, 1, c["result"]) + block + exp
    recs = _sweep(("front", "lz4"), NC.front_cases("lz4"), lambda p, n, cap, out: L.sim_lz4_wave_decode(p, n, out, cap, 0), rec, rings=("own",))
    _sanitized(tmp_path, "sim_lz4_wave.cpp", recs)
    rec = lambda c, mis, block, exp: struct.pack("<3Iq", len(c["bytes"]), c["cap"], mis & 3, c["result"]) + block + exp
    recs = _sweep(("front", "snappy"), NC.front_cases("snappy"), lambda p, n, cap, out: Ls.sim_snappy_wave_decode(p, n, out, cap), rec, rings=("own",))
    _sanitized(tmp_path, "sim_snappy_wave.cpp", recs)


def test_bgzf_walk(sims, tmp_path):
    """the hop walk is host code (cramjam_amd/csrc/bgzf_grammar.hpp) that reads memory as it is: every cut in place under every ring —
    under `own` the rest of a valid member follows the cut — gives the model's code and members; the members' DEFLATE streams are the
    gzip cases above"""
    import bgzf_model as B
    L = sims["bgzf"]
    cases = NC.bgzf_size_cases()                    # one per cut, each at offsets 0, 1, 2 and 3 modulo 4
    walks = {}
    recs = []
    for ring in NC.RINGS:
        blob, off, _, _ = NC.case_layout("bgzf-walk", cases, ring)
        Bl = Blob(blob, off)
        assert not NC.alignment_coverage(cases, off), (ring, NC.alignment_coverage(cases, off))
        for i, c in enumerate(cases):
            if (c["base"], c["k"]) not in walks:
                walks[(c["base"], c["k"])] = B.walk(c["bytes"])
            code, mem = walks[(c["base"], c["k"])]
            rows, n = (C.c_ulonglong * (3 * len(mem) + 3))(), C.c_ulonglong()
            assert L.sim_bgzf_walk(Bl.at(i), len(c["bytes"]), rows, len(mem) + 1, C.byref(n)) == code, (ring, c["base"], c["k"])
            assert n.value == len(mem) and list(rows)[:3 * len(mem)] == [x for m in mem for x in m], (ring, c["base"], c["k"])
            assert (code or sum(m[2] for m in mem)) == c["size"]
            if ring == "zero":
                recs.append(struct.pack("<IIq", len(c["bytes"]), len(mem), code) + c["bytes"] + b"".join(struct.pack("<3Q", *m) for m in mem))
    exe = build_sim("sim_bgzf_grammar.cpp", str(tmp_path / "sim_bgzf_main"), main=True, sanitize=True)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "%d cases, 0 bad" % len(recs) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_blosclz_stream_decoder_inside_its_chunk(sims, tmp_path):
    """every BloscLZ stream of the fixture, malformed and hand-written chunks decoded in place: its neighbours are the chunk's own
    bytes — the stream table in front of the first, the next stream behind each — and around the chunk the ring's"""
    import blosc_model as BM
    import blosclz_model as Z
    L = sims["blosclz"]
    _, chunks = NC.blosc_cases("blosclz")
    chunks = [c for c in chunks if Z.is_blosclz(c["bytes"])]
    recs, runs, straddle = [], 0, 0
    for ring in NC.RINGS:
        blob, off, _, _ = NC.case_layout("blosclz-model", chunks, ring)
        B = Blob(blob, off)
        for i, c in enumerate(chunks):
            try:
                table = Z.parse(c["bytes"])[1]
            except BM.Refused:
                continue
            for src, ln, _d, dlen, _b, stored in table:
                if stored:
                    continue
                s = c["bytes"][src:src + ln]
                try:
                    want = Z.decode_stream(s, dlen)
                except BM.Refused:
                    want = None
                out = (C.c_ubyte * max(dlen, 1))()
                r = L.sim_blosclz_decode(B.at(i) + src, ln, out, dlen)
                assert r != SIM_BOUNDS and r == (-7 if want is None else dlen), (ring, c["base"], src, r)
                assert want is None or bytes(out[:dlen]) == want, (ring, c["base"], src)
                at = B.off[i] + src
                runs += 1
                straddle += (at + ln) % 4 != 0
                front = at & 3                                        # every run goes to the sanitizer program too
                recs.append(struct.pack("<3Iq", ln, dlen, front, r) + C.string_at(B.base + at - front, (front + ln + 3) & ~3) + (want or b""))
    assert runs > 4 * 1000 and 4 * straddle >= runs
    _sanitized(tmp_path, "sim_blosclz_decode.cpp", recs)


def test_zlib_and_zstd_streams_inside_their_blosc_chunks(sims):
    """the streams of the Zlib- and Zstd-format Blosc chunks (fixtures, malformed, hand-written) through the DEFLATE and Zstandard
    decoders in place, at the capacity the chunk's table states: what tests/blosc_zcodec_model.py says of each stream (zlib live;
    libzstd where it is loaded, else an accepted fixture's streams must come out whole), and the SAME result and bytes under every ring"""
    import blosc_model as BM
    import blosc_zcodec_model as Z
    try:
        import zstd_cases
        zstd_cases.libzstd()
        have_zstd = True
    except OSError:
        have_zstd = False
    Ld, Lz = sims["deflate"], sims["zstd"]
    _, chunks = NC.blosc_cases("zcodecs")
    chunks = [c for c in chunks if Z.fmt_of(c["bytes"]) is not None]
    first, runs = {}, 0
    for ring in NC.RINGS:
        blob, off, _, _ = NC.case_layout("zcodecs-model", chunks, ring)
        B = Blob(blob, off)
        for i, c in enumerate(chunks):
            fmt = Z.fmt_of(c["bytes"])
            try:
                table = Z.parse(c["bytes"])[1]
            except BM.Refused:
                continue
            for src, ln, _d, dlen, _b, stored in table:
                if stored:
                    continue
                out = (C.c_ubyte * max(dlen, 1))()
                if fmt == Z.FORMAT_ZLIB:
                    r = Ld.sim_deflate_decode(DF.ZLIB, 0, B.at(i) + src, ln, out, dlen)
                else:
                    r = Lz.sim_zstd_decode(0, B.at(i) + src, ln, out, dlen)
                got = bytes(out[:dlen]) if r == dlen else None
                assert r != SIM_BOUNDS, (ring, c["base"], src)
                assert first.setdefault((i, src), (r, got)) == (r, got), (ring, c["base"], src, r, first[(i, src)][0])
                if fmt == Z.FORMAT_ZLIB or have_zstd:
                    try:
                        want = Z.decode_stream(fmt, c["bytes"][src:src + ln], dlen)
                    except BM.Refused:
                        want = None
                    assert got == want, (ring, c["base"], src, r)
                elif c["result"] >= 0:
                    assert r == dlen, (ring, c["base"], src, r)
                runs += 1
    assert runs >= 4 * 300 and sum(1 for r, got in first.values() if got is None) >= 10


# ---- the inputs bite ---------------------------------------------------------------------------------------------------------------------------
def _bites(name, s, verdict):
    """with in_len overstated by 3 the ring's first bytes count as stream: at some cut the verdicts under own, ff and zero differ"""
    for k in range(len(s) + 1):
        own = NC.own_of_cut(s, k)[1][:3]
        if len({verdict(s[:k] + tail) for tail in (own, b"\xff\xff\xff", b"\0\0\0")}) > 1:
            return
    assert False, name


def test_the_rings_bite_when_in_len_is_overstated_by_three(sims):
    import bgzf_model as B
    import lz4_dict_model as D
    for wrap in DF.WRAPS:
        for name, s in NC.deflate_bases(wrap):
            _bites(name, s, lambda x: DF.verdict(wrap, x, 364))
    Lz = sims["zstd"]

    def zstd(x, cap):
        buf, out = C.create_string_buffer(x, len(x) + 4), (C.c_ubyte * (cap + 1))()
        r = Lz.sim_zstd_decode(0, C.addressof(buf), len(x), out, cap)
        return r, bytes(out[:max(r, 0)])
    for name, s, U in NC.zstd_base_streams():
        _bites(name, s, lambda x: zstd(x, U + 64))
    d = D.dictionary(NC.DICT_LEN)
    bases = {}
    for c in NC.lz4_dict_cases():
        bases.setdefault(c["base"], []).append(c)
    for name, cs in bases.items():
        full = max(cs, key=lambda c: c["k"])
        assert any(len({D.decode(c["bytes"] + tail, full["cap"], d) for tail in (c["own"][1][:3], b"\xff\xff\xff", b"\0\0\0")}) > 1 for c in cs if c["cap"] == full["cap"]), name
    for name, s in NC.bgzf_bases():
        _bites(name, s, lambda x: B.walk(x)[0])


# ---- the encoders' inputs and expectations -----------------------------------------------------------------------------------------------------
def test_encoder_inputs_are_flanked_by_their_own_period():
    cs = NC.encoder_inputs()
    assert {c["period"] for c in cs} == set(NC.PERIODS) | {0} and {len(c["bytes"]) for c in cs} == set(NC.LENGTHS)
    assert len(cs) == (len(NC.PERIODS) + 1) * len(NC.LENGTHS)
    for c in cs:
        f, b = c["own"]
        x, p = f + c["bytes"] + b, c["period"]
        assert len(f) == len(b) == NC.M
        if p:
            assert all(x[i] == x[i + p] for i in range(len(x) - p)), c["name"]                  # one period from 64 bytes below 0 to 64 behind n
            assert p == 1 or any(x[i] != x[i + q] for q in range(1, p) for i in range(min(len(x) - q, 2 * p))), c["name"]      # ... and no shorter one
        else:
            n = len(c["bytes"])
            assert b[:min(n, 32)] == c["bytes"][-32:] and f[-min(n, 64):] == c["bytes"][-64:], c["name"]
    blob, off, fronts, behinds = NC.layout([c["bytes"] for c in cs], "own", [c["own"] for c in cs], [c["mis"] for c in cs])
    assert all(fr == c["own"][0] and be == c["own"][1] for c, fr, be in zip(cs, fronts, behinds))
    assert {int(o) % 16 for o in off} == set(range(16))
    for ring in NC.RINGS:                                             # every layout holds every input, with its margins
        blob, off, _, _ = NC.layout([c["bytes"] for c in cs], ring, [c["own"] for c in cs], [c["mis"] for c in cs])
        assert int(off.min()) >= NC.M and all(int(o) + len(c["bytes"]) + NC.M <= len(blob) for o, c in zip(off, cs))
        assert all(blob[int(o):int(o) + len(c["bytes"])].tobytes() == c["bytes"] for o, c in zip(off, cs))
        assert {int(o) % 16 for o in off} == set(range(16)), ring


def test_encoder_models_streams_decode_to_their_inputs(sims):
    """... by the oracle, zlib, the dictionary model and the host build of the Zstandard decoder; where liblz4 and libzstd are loaded,
    the dictionary streams and the frames by them as well: references that are none of the project's"""
    import lz4_dict_model as D
    import oracle
    import zstd_cases as Z
    raws = [c["bytes"] for c in NC.encoder_inputs()]
    d = D.dictionary(NC.DICT_LEN)
    Lz = sims["zstd"]
    lz4 = D.liblz4()
    try:
        Z.libzstd()
        zstd = True
    except OSError:
        zstd = False
    for codec in NC.ENCODERS:
        for raw, (cap, s) in zip(raws, NC.encoder_expected(codec)):
            n = len(raw)
            if codec == "lz4":
                got = oracle.lz4_decompress_raw(s, n)
            elif codec == "snappy":
                got = oracle.snappy_decompress(s)
            elif codec == "lz4_dict":
                got = D.decode(s, n, d)
                assert lz4 is None or D.lz4_decode_using_dict(lz4, s, n, d) == (n, raw), (codec, n)
            elif codec.startswith("deflate"):
                got = n, zlib.decompress(s, DF.WBITS[NC.ENCODERS.index(codec) - 3])
            else:
                buf, out = C.create_string_buffer(s, len(s) + 4), (C.c_ubyte * n)()
                got = Lz.sim_zstd_decode(0, C.addressof(buf), len(s), out, n), bytes(out)
                assert not zstd or Z.zstd_verdict(s, n) == (n, raw), (codec, n)
            assert (got[0], bytes(got[1])) == (n, raw), (codec, n)
