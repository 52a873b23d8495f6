"""The Zstandard encoder on the CPU: the scalar model (tests/hostsim/zstd_enc_model.c) read back by libzstd and by the
host build of the project's own decoder; the host build of the kernel's entropy stage (tests/hostsim/sim_zstd_encode.cpp, every access
bounds-checked) against the model byte for byte on every case of tests/zstd_enc_cases.py at three input and output alignments at the
bound, and at capacities exact, exact - 1 and 0 at one of them each, with guard bytes behind every capacity; what the cases were built
to reach, asserted on the model's records and report; the encode tables against the decode tables of tests/zstd_cases.py; the bound;
the ratio over the corpus.  No GPU.

One-off, not a committed test: the host build as a stand-alone program under -fsanitize=address,undefined on exact-size heap blocks over
the file of tests/zstd_enc_cases.write_cases_file() (every case x both flags x four capacities); its docstring has the commands."""
import ctypes as C
import os

import pytest

import zstd_cases as Z
import zstd_enc_cases as E
from hostsim_build import build_sim

ALIGN = ((0, 0), (1, 5), (3, 15))       # (input, output) bytes behind a 16-byte boundary


def _libzstd():
    try:
        L = Z.libzstd()
    except OSError as ex:
        pytest.skip("no libzstd on this machine: %s" % ex)
    L.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    L.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    return L


def test_libzstd_reads_the_models_frames():
    L = _libzstd()
    for name, data in E.cases().items():
        for flags in E.FLAGS:
            r, s, _ = E.model(data, flags)
            assert r == len(s) and 0 < r <= E.bound(len(data), flags), (name, flags, r)
            assert Z.zstd_verdict(s, len(data)) == (len(data), data), (name, flags)
            assert L.ZSTD_getFrameContentSize(s, len(s)) == len(data), name
            assert (s[4] >> 2) & 1 == flags
        if len(data) > 8:           # the checksum is read: a frame whose last byte is off is refused
            s = bytearray(E.model(data, 1)[1])
            s[-1] ^= 1
            assert Z.zstd_verdict(bytes(s), len(data))[0] == Z.ERROR_FAMILY[22], name


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simzd") / "libsimz.so")
    S = C.CDLL(build_sim(os.path.join(E.SIM, "sim_zstd_decode.cpp"), so))
    S.sim_zstd_decode.restype = C.c_longlong
    S.sim_zstd_decode.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    return S


def test_the_projects_decoder_reads_the_models_frames(decoder):
    tags = set()
    for name, data in E.cases().items():
        for flags in E.FLAGS:
            s = E.model(data, flags)[1]
            src = C.create_string_buffer(s + b"\x77", len(s) + 1)
            out = C.create_string_buffer(b"\xa5" * (len(data) + 64), len(data) + 64)
            assert decoder.sim_zstd_decode(0, src, len(s), out, len(data)) == len(data), (name, flags)
            assert out.raw[:len(data)] == data and out.raw[len(data):] == b"\xa5" * 64, (name, flags)
            assert decoder.sim_zstd_decode(1, src, len(s), None, 0) == len(data), (name, flags)
            tags |= Z.classify(s) | Z.deep_classify(s)
    # what the frames claim, found by the decoder's own reader
    want = {"frame:checksum", "frame:nochecksum", "frame:single", "frame:window", "wd:0x30", "fcs:1", "fcs:2", "fcs:4", "block:raw", "block:rle",
            "block:compressed", "lit:raw", "lit:huf1", "lit:huf4", "weights:direct", "weights:fse", "huf:2symbols", "huf:256symbols", "huf:log11", "w:log5",
            "lh:raw0", "lh:raw1", "lh:raw3", "lh:huf0", "lh:huf2", "lh:huf3", "nseq:0", "nseq:1byte", "nseq:2byte", "off:new", "off:rep1"}
    want |= {"%s:%s" % (t, m) for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse")}
    assert want <= tags, sorted(want - tags)
    assert not tags & {"lit:treeless", "ll:repeat", "of:repeat", "ml:repeat", "off:rep2", "off:rep3"}


def test_host_build_emits_the_models_bytes_at_every_alignment_and_capacity():
    runs = 0
    for k, (name, data) in enumerate(E.cases().items()):
        for flags in E.FLAGS:
            r, s, rep = E.model(data, flags)
            for im, om in ALIGN:
                got = E.sim(data, flags, E.bound(len(data), flags), im, om)
                assert got[:2] == (r, s) and got[2] == [p[:E.SIM_INFO] for p in rep], (name, flags, im, om)
                runs += 1
            im, om = ALIGN[(k + flags + 1) % 3]
            assert E.sim(data, flags, r, im, om)[:2] == (r, s), (name, flags, "exact")
            assert E.sim(data, flags, r - 1, im, om)[0] == E.OUT_TOO_SMALL, (name, flags, "exact - 1")
            assert E.sim(data, flags, 0, im, om)[0] == E.OUT_TOO_SMALL, (name, flags, 0)
            assert E.model(data, flags, r - 1)[0] == E.OUT_TOO_SMALL and E.model(data, flags, r)[0] == r
    assert runs >= 3 * len(E.cases())


def test_the_coverage_matrix():
    cov = E.coverage()
    assert cov["block"] == {E.RAW, E.RLE, E.COMPRESSED} and cov["head"] == {6, 7, 8, 10}
    # a Compressed block's literals are never in RLE mode while the pieces are independent: every byte value of a piece is a literal at
    # its first occurrence, so one distinct literal means one distinct byte, which is an RLE block
    assert cov["lit"] == {E.RAW, E.HUF} and cov["streams"] == {1, 4} and cov["tree"] == {E.DIRECT, E.FSE_WEIGHTS}
    assert cov["lit_header"] == {(E.RAW, 1), (E.RAW, 2), (E.RAW, 3), (E.HUF, 3), (E.HUF, 4), (E.HUF, 5)}
    assert cov["nseq_form"] == {0, 1, 2}
    assert cov["ll"] == cov["of"] == cov["ml"] == {E.PREDEFINED, E.RLE_MODE, E.FSE_MODE}
    cs = E.cases()
    rep = lambda k: E.model(cs[k])[2]
    for T in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384):
        assert rep("lits%d" % T)[0][7] == T and rep("lits%d" % T)[0][9] == E.COMPRESSED, T
    assert rep("lits1023")[0][:2] == (E.HUF, 1) and rep("lits1024")[0][:2] == (E.HUF, 4)
    assert [rep("seq%d" % n)[0][6] for n in (0, 1, 127, 128)] == [0, 1, 127, 128] and rep("seq0")[0][9] == E.COMPRESSED
    assert [p[9] for p in rep("text_random_text")] == [E.COMPRESSED, E.RAW, E.COMPRESSED]
    assert [p[9] for p in rep("one131073")] == [E.RLE] * 3 and len(cs["one131073"]) % E.PIECE == 1
    for n in (255, 256, 65535, 65536, 65537, 65791, 65792):       # Raw blocks: the bound is met with equality (a last piece of one byte
        r, s, p = E.model(cs["random%d" % n], 1)                   # is an RLE block of a Raw block's size)
        assert r == E.bound(n, 1) and p[0][9] == E.RAW and all(x[9] != E.COMPRESSED for x in p), n
    assert rep("huf_two")[0][0] == E.HUF and rep("huf_two")[0][11] == 2
    assert rep("huf_equal128")[0][0] == E.HUF and rep("huf_equal128")[0][11] == 128 and max(cs["huf_equal128"]) == 128
    assert rep("huf_fibonacci")[0][0] == E.HUF and rep("huf_fibonacci")[0][10] > 11           # the limit cuts the tree
    assert max(cs["text4k"]) < 128 and rep("text4k")[0][0] == E.HUF
    # all 256 symbols with skewed counts: direct weights cannot say them, this takes FSE-compressed weights
    assert len(set(cs["huf_skewed256"])) == 256 and rep("huf_skewed256")[0][:3] == (E.HUF, 4, E.FSE_WEIGHTS)
    assert rep("huf_equal128")[0][2] == E.FSE_WEIGHTS and rep("huf_direct127")[0][:3] == (E.HUF, 4, E.DIRECT)     # 127 equal weights: one distinct symbol
    assert rep("lits31")[0][9] == E.COMPRESSED and rep("lits31")[0][0] == E.RAW and len(set(cs["lits31"])) == 31  # a tree would cost more than it saves
    assert rep("fse_rle")[0][3:7] == (E.PREDEFINED, E.RLE_MODE, E.RLE_MODE, 6)
    short, long_ = rep("fse_predefined")[0], rep("fse_all")[0]
    assert short[3:6] == (E.PREDEFINED,) * 3 and short[6] >= 8 and len(cs["fse_predefined"]) < 1500      # a short piece: Predefined wins
    assert long_[3:6] == (E.FSE_MODE,) * 3 and len(cs["fse_all"]) >= 3000                                  # a long one: FSE_Compressed, all three
    assert sorted(E.bit_offset_texts()) == list(range(8))


def test_exact_lengths_and_distances_from_the_records():
    cs = E.cases()
    for b in E.ML_BASES:
        for L in (b - 1, b):
            assert [r for r in E.records(cs["mlen%d" % L]) if r[3]] == [(0, 600, 600, L)], L
    for b in E.LL_BASES:
        for L in (b - 1, b):
            assert any(r[1] == L and r[3] for r in E.records(cs["llen%d" % L])), L
    for d in E.DISTANCES:
        assert len(cs["dist%d" % d]) <= E.PIECE and any(r[2] == d and r[3] >= 4 for r in E.records(cs["dist%d" % d])), d
    assert {1, 4, 5, 12, 13, 32764, 32765, 65000} <= set(E.DISTANCES)


def test_the_repeat_code_from_the_records():
    cs = E.repeat_cases()
    a, b = [r for r in E.records(cs["rep_between"]) if r[3]][:2]
    assert a[2] == b[2] == 700 and b[1] == 5                                  # two matches at one distance, literals between them
    assert "off:rep1" in Z.deep_classify(E.model(cs["rep_between"])[1])
    first = E.records(cs["rep_first"])[0]
    assert first[2] == 1 and first[1] > 0 and first[3] > 4                    # the frame's first sequence at distance 1: the initial history
    assert Z.deep_classify(E.model(cs["rep_first"])[1]) >= {"off:rep1"} and "off:new" not in Z.deep_classify(E.model(cs["rep_first"])[1])
    one, two = cs["rep_split"][:E.PIECE], cs["rep_split"][E.PIECE:]
    assert [r for r in E.records(one) if r[3]][-1][2] == 700 and E.records(two)[0][1:3] == (700, 700)      # the pair split across two pieces
    rep = E.model(cs["rep_split"])[2]
    assert rep[0][9] == rep[1][9] == E.COMPRESSED and rep[1][4] == E.RLE_MODE  # ... the second piece's one offset code is the repeat code
    assert "off:rep1" in Z.deep_classify(E.model(cs["rep_split"])[1])
    # a literal length of 0 takes the raw offset whatever the distance: text has such sequences
    assert any(r[1] == 0 and r[3] for r in E.records(E.cases()["text4k"]))
    # across a Raw block the history stays: the third piece of text | random | text starts from the first piece's last distance
    t = E.cases()["text_random_text"]
    assert [r for r in E.records(t[:E.PIECE]) if r[3]][-1][2] > 0


# ---- the encode tables against the decode tables of tests/zstd_cases.py --------------------------------------------------------------
def _walks(st, dnb, dfs, log, counts, name):
    """from every state, coding any used symbol leaves bits and a next state from which the decoder's cell gives back that symbol, that
    many bits and, with the bits, the state that was left"""
    size, cells = 1 << log, Z.fse_cells(log, counts)
    assert sorted(st[:size]) == list(range(size, 2 * size)), name
    for s, c in enumerate(counts):
        if c == 0:
            continue
        reached = set()
        for x in range(size, 2 * size):
            nb = (x + dnb[s]) >> 16
            nxt = st[(x >> nb) + dfs[s]]
            sym, bits, base = cells[nxt - size]
            assert (sym, bits) == (s, nb) and base + (x & ((1 << nb) - 1)) == x - size, (name, s, x)
            reached.add(nxt)
        assert len(reached) == abs(c), (name, s)


def _histograms(nsym):
    yield "huge_and_ones", [16000] + [1] * (nsym - 1)
    yield "equal", [7] * nsym
    yield "two", [0, 5] + [0] * (nsym - 3) + [1]
    yield "two_first", [900, 100] + [0] * (nsym - 2)
    g = E.D._lcg(nsym)
    yield "random", [next(g) % 1000 if next(g) % 3 else 0 for _ in range(nsym)]
    yield "random_small", [next(g) % 4 for _ in range(nsym - 1)] + [1]


@pytest.mark.parametrize("name,nsym,maxlog", [("ll", 36, 9), ("of", 29, 8), ("ml", 53, 9), ("weights", 12, 6)])
def test_normaliser_ncount_and_table_builder_alone(name, nsym, maxlog):
    """the normaliser, the NCount writer and the table builder as the kernel's lanes call them, for all four alphabets: the counts sum to
    the table's size, every used symbol is present, and tests/zstd_cases.py's own read_ncount / fse_cells rebuild from the written
    description the decode table that the encode table walks"""
    L = E.lib()
    for hname, hist in _histograms(nsym):
        total = sum(hist)
        h = (C.c_uint32 * nsym)(*hist)
        norm, nc, ncb = (C.c_int16 * 64)(), (C.c_ubyte * 96)(), C.c_uint(0)
        st, dnb, dfs = (C.c_uint16 * 512)(), (C.c_uint32 * 64)(), (C.c_int32 * 64)()
        log = L.sim_zsf_table(h, nsym, maxlog, total, norm, nc, C.byref(ncb), st, dnb, dfs)
        top = max(s for s in range(nsym) if hist[s])
        counts = list(norm[:top + 1])
        assert 5 <= log <= maxlog and sum(counts) == 1 << log, (name, hname, log)
        assert all((c >= 1) == (hist[s] > 0) for s, c in enumerate(counts)), (name, hname)
        rlog, rcounts, used = Z.read_ncount(bytes(nc[:ncb.value]) + bytes(8), nsym - 1, set())
        assert (rlog, rcounts, used) == (log, counts, ncb.value) and ncb.value <= 96, (name, hname, rlog, used)
        _walks(st, dnb, dfs, log, counts, (name, hname))


@pytest.mark.parametrize("t,name", [(0, "ll"), (1, "of"), (2, "ml")])
def test_predefined_encode_tables_walk_the_decoders_cells(t, name):
    log, counts = Z._DEFAULTS[name]
    st, dnb, dfs = (C.c_uint16 * 512)(), (C.c_uint32 * 64)(), (C.c_int32 * 64)()
    assert E.lib().sim_zse_table(t, st, dnb, dfs) == log and all(counts)
    _walks(st, dnb, dfs, log, counts, name)
    for s in range(len(counts)):                                           # the opening state: libzstd's FSE_initCState2
        nb0 = (dnb[s] + (1 << 15)) >> 16
        assert Z.fse_cells(log, counts)[st[(((nb0 << 16) - dnb[s]) >> nb0) + dfs[s]] - (1 << log)][0] == s, (name, s)


def test_bound():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    L = N.lib()
    for n in (0, 1, 255, 256, 65535, 65536, 65537, 65791, 65792, 131072, 200000, 0x7E000000):
        for flags in E.FLAGS:
            b = L.cj_zstd_compress_bound(n, flags)
            head = 6 if n <= 255 else 7 if n <= 65536 else 8 if n <= 65791 else 10
            assert b == E.bound(n, flags) == E.lib().sim_zse_bound(n, flags) == head + 3 * max(1, -(-n // 65536)) + n + 4 * flags
            assert b <= n + 3 * (n // 65536 + 1) + 14
    assert L.cj_zstd_compress_bound(0x7E000001, 0) == 0 and L.cj_zstd_compress_bound(10, 2) == 0 and E.bound(10, 2) == 0
    assert batch.zstd_compress_bound(0) == 9 and batch.zstd_compress_bound(100, checksum=True) == 113


def test_argument_refusals_that_need_no_device():
    from cramjam_amd import _native as N
    L = N.lib()
    dev = lambda fmt, flags, n=0: L.cj_zstd_compress_batch_device(None, fmt, flags, n, None, None, None, None, None, None, None, None)
    host = lambda fmt, flags, n=0: L.cj_zstd_compress_batch_host(None, fmt, flags, n, None, None, None, None, None)
    for call in (dev, host):
        for flags in E.FLAGS:
            assert call(N.ZSTD_FRAMES, flags) == 0                        # n == 0 succeeds
            assert call(N.ZSTD_FRAMES, flags, 3) == E.BAD_ARG             # a batch without its pointers
        for flags in (2, 3, 0x100, 0x80000000):
            assert call(N.ZSTD_FRAMES, flags) == E.BAD_ARG, flags
        assert call(1, 0) == E.BAD_ARG and call(-1, 0) == E.BAD_ARG
    assert L.cj_zstd_batch_device(None, N.ZSTD_FRAMES, N.OP_COMPRESS, 0, 0, None, None, None, None, None, None, None, None) == E.BAD_ARG


# ---- the ratio over the corpus, on the model -------------------------------------------------------------------------------------------
# bytes of this encoder / bytes of libzstd level 1 (per 64 KiB chunk), per file, rounded up to the next whole percent
PINNED = {"Mark.Twain-Tom.Sawyer.txt": 1.03, "alice29.txt": 1.03, "asyoulik.txt": 1.02, "dickens.sample64k": 1.03, "fireworks.jpeg": 1.00,
          "geo.protodata": 1.11, "html": 1.08, "html_x_4": 1.08, "kppkn.gtb": 1.31, "lcet10.txt": 1.04, "mr.sample64k": 1.01,
          "nci.sample64k": 1.35, "ooffice.sample64k": 1.00, "osdb.sample64k": 1.01, "paper-100k.pdf": 1.00, "plrabn12.txt": 1.02,
          "reymont.sample64k": 1.12, "urls.10K": 1.07, "x-ray.sample64k": 0.97, "xml.sample64k": 1.13}
PINNED_TOTAL = 1.03
DEFLATE_MODEL_TOTAL = 3746370           # tests/test_deflate_encode_model.py's encoder on the same chunks (raw streams)


def test_ratio_over_the_corpus():
    _libzstd()
    from test_enc2_model import model_lib, model_lz4
    lz4 = model_lib()
    total = total_zstd = total_lz4 = 0
    seen = set()
    for f in E.corpus_files():
        name = os.path.basename(f)[:-4]
        a = z = l4 = 0
        for c in E.corpus_chunks(f):
            a += E.model(c)[0]
            z += len(Z.zstd_compress(c, level=1))
            l4 += len(model_lz4(lz4, c))
        print("%-28s this %8d zstd-1 %8d ratio %.4f lz4 model %8d" % (name, a, z, a / z, l4))
        assert a <= PINNED[name] * z, (name, a / z)
        seen.add(name)
        total += a; total_zstd += z; total_lz4 += l4
    print("total: this %d zstd-1 %d (%.4f) lz4 model %d deflate model %d" % (total, total_zstd, total / total_zstd, total_lz4, DEFLATE_MODEL_TOTAL))
    assert seen == set(PINNED)
    assert total <= PINNED_TOTAL * total_zstd and total < total_lz4 and total < DEFLATE_MODEL_TOTAL
