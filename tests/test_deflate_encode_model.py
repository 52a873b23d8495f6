"""The DEFLATE encoder on the CPU: the scalar model (tests/hostsim/deflate_enc_model.c) against Python's zlib, the host
build of the kernel's entropy stage (tests/hostsim/sim_deflate_encode.cpp, every access bounds-checked) against the model byte for
byte on every case of tests/deflate_enc_cases.py at three input and three output alignments at the bound, and at capacities exact,
exact - 1 and 0 at one of them each, with guard bytes behind every capacity; what the cases were built to reach, asserted on the model's records, block types and tree
depths; the code builder alone against a package-merge of the test's own; the ratio over the corpus.  No GPU."""
import ctypes as C
import gzip
import os
import zlib

import pytest

import deflate_cases as D
import deflate_enc_cases as E

ALIGN = ((0, 0), (1, 5), (3, 15))       # (input, output) bytes behind a 16-byte boundary


def test_model_streams_inflate_with_zlib():
    for name, data in E.cases().items():
        for wrap in E.WRAPS:
            r, s, types, info = E.model(data, wrap)
            assert r == len(s) and 0 < r <= E.bound(len(data), wrap), (name, wrap, r)
            d = zlib.decompressobj(E.WBITS[wrap])
            assert d.decompress(s) == data and d.eof and d.unused_data == b"", (name, wrap)
        assert gzip.decompress(E.model(data, E.GZIP)[1]) == data, name


def test_host_build_emits_the_models_bytes_at_every_alignment_and_capacity():
    runs = 0
    for k, (name, data) in enumerate(E.cases().items()):
        for wrap in E.WRAPS:
            r, s, _, _ = E.model(data, wrap)
            for im, om in ALIGN:
                assert E.sim(data, wrap, E.bound(len(data), wrap), im, om) == (r, s), (name, wrap, im, om)
                runs += 1
            im, om = ALIGN[(k + wrap + 1) % 3]
            assert E.sim(data, wrap, r, im, om) == (r, s), (name, wrap, "exact")
            assert E.sim(data, wrap, r - 1, im, om)[0] == E.OUT_TOO_SMALL, (name, wrap, "exact - 1")
            assert E.sim(data, wrap, 0, im, om)[0] == E.OUT_TOO_SMALL, (name, wrap, 0)
            assert E.model(data, wrap, r - 1)[0] == E.OUT_TOO_SMALL and E.model(data, wrap, r)[0] == r
    assert runs >= 3 * len(E.cases())


def test_exact_match_lengths_reach_the_split_rule():
    for L in E.MATCH_LENGTHS:
        recs = [r for r in E.records(E.match_length_case(L)) if r[3]]
        assert recs == [(0, 600, 600, L)], (L, recs)
    # ... and the split itself, read back from the stream: pieces of at most 258, none below 3
    for L, want in ((258, [258]), (259, [256, 3]), (260, [257, 3]), (261, [258, 3]), (262, [258, 4]), (516, [258, 258]), (517, [258, 256, 3]), (520, [258, 258, 4])):
        assert _match_lengths(E.model(E.match_length_case(L), E.RAW)[1]) == want, L
    zeros = [r for r in E.records(bytes(E.PIECE)) if r[3]]
    assert sum(r[3] for r in zeros) > 65000 and max(r[3] for r in zeros) > 258


def test_exact_match_distances_and_the_window():
    for name, (d, data) in E.distance_cases().items():
        recs = E.records(data)
        if name.startswith("dist"):
            assert any(r[2] == d and r[3] >= 16 for r in recs), name
        else:
            assert all(r[2] != d for r in recs), name
        assert all(r[2] <= 32768 for r in recs), name
    assert set(E.DISTANCES) >= {1, 2, 4, 5, 8, 9, 24576, 24577, 32767, 32768} and all(d > 32768 for d in E.TOO_FAR)


def test_the_length_limit_is_reached():
    assert E.model(E.fibonacci_piece(), E.RAW)[3][0] > 15
    deep = E.deep_corpus_chunks()
    print("corpus chunks deeper than 15:", [n for n, _ in deep])
    assert len(deep) >= 1


def test_block_choice_and_bit_carry_over():
    for n in (65535, 65536, 65537):
        r, s, types, _ = E.model(D.random_bytes(n, 3), E.RAW)
        assert types[0] == E.STORED and s[0] & 7 == (1 if n == 65535 else 0), n
    assert E.model(D.random_bytes(65536, 3), E.RAW)[0] == 65536 + 10 == E.bound(65536, E.RAW)      # two stored blocks
    assert E.model(E.three_pieces(), E.RAW)[2] == [E.DYNAMIC, E.STORED, E.DYNAMIC]
    r, s, types, _ = E.model(E.fixed_text(), E.RAW)
    assert len(E.fixed_text()) == 300 and types == [E.FIXED] and s[0] & 7 == 3           # BFINAL 1, BTYPE 01
    assert E.model(b"", E.RAW)[1] == b"\x03\x00" and E.model(b"", E.RAW)[2] == [E.FIXED]
    ends = E.bit_offset_texts()
    assert sorted(ends) == list(range(8))
    for off, t in ends.items():
        s = E.model(t, E.RAW)[1]
        assert off == 0 or s[-1] >> off == 0, off                                        # the pad bits are 0


def test_bound():
    from cramjam_amd import _native as N
    L = N.lib()
    for n in (0, 1, 65535, 65536, 65537, 131072, 200000, 0x7E000000):
        for wrap in E.WRAPS:
            b = L.cj_deflate_compress_bound(n, wrap)
            assert b == E.bound(n, wrap) == E.lib().sim_dfe_bound(n, wrap)
            assert b <= n + 10 * (n // 65536 + 1) + 18
    assert L.cj_deflate_compress_bound(0x7E000001, 0) == 0 and L.cj_deflate_compress_bound(10, 3) == 0
    for wrap, extra in ((E.RAW, 0), (E.ZLIB, 6), (E.GZIP, 18)):              # the worst case is met: a full piece that is stored
        assert E.model(D.random_bytes(65536, 3), wrap)[0] == 65536 + 10 + extra == E.bound(65536, wrap)


def test_argument_refusals_that_need_no_device():
    from cramjam_amd import _native as N
    from cramjam_amd import batch
    L = N.lib()
    dev = lambda wrap, flags, n=0: L.cj_deflate_compress_batch_device(None, wrap, flags, n, None, None, None, None, None, None, None, None)
    host = lambda wrap, flags, n=0: L.cj_deflate_compress_batch_host(None, wrap, flags, n, None, None, None, None, None)
    for call in (dev, host):
        for wrap in E.WRAPS:
            assert call(wrap, 0) == 0                                     # n == 0 succeeds
            for flags in (1, 2, 0x100, 0x80000000):
                assert call(wrap, flags) == E.BAD_ARG, flags
            assert call(wrap, 0, 3) == E.BAD_ARG                          # a batch without its pointers
        assert call(3, 0) == E.BAD_ARG and call(-1, 0) == E.BAD_ARG
    assert batch.deflate_compress_bound(100, "gzip") == 123 and batch.deflate_compress_bound(0) == 5
    with pytest.raises(ValueError):
        batch.deflate_compress_bound(1, wrapper="lzma")
    with pytest.raises(ValueError):
        batch.deflate_compress_many([b"x"], wrapper="deflate64")


# ---- reading a raw stream of this encoder back: the match lengths in stream order (fixed or dynamic blocks) ------------------------------
def _match_lengths(s):
    bits = "".join(format(b, "08b")[::-1] for b in s)
    pos = 0

    def take(n):
        nonlocal pos
        v = int(bits[pos:pos + n][::-1] or "0", 2)
        pos += n
        return v

    def decoder(lens):
        codes, code = {}, 0
        for ln in range(1, 16):
            for sym, l in enumerate(lens):
                if l == ln:
                    codes[(ln, code)] = sym
                    code += 1
            code <<= 1

        def sym():
            nonlocal pos
            c = 0
            for ln in range(1, 16):
                c = (c << 1) | int(bits[pos]); pos += 1
                if (ln, c) in codes:
                    return codes[(ln, c)]
            raise AssertionError("bad code")
        return sym
    out = []
    while True:
        final, btype = take(1), take(2)
        assert btype in (1, 2)
        if btype == 1:
            ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = take(3)
            nxt, lens = decoder(cl), []
            while len(lens) < hlit + hdist:
                v = nxt()
                if v < 16:
                    lens.append(v)
                elif v == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * ((3 + take(3)) if v == 17 else (11 + take(7)))
            ll, dl = lens[:hlit], lens[hlit:]
        lit, dist = decoder(ll), decoder(dl)
        while True:
            v = lit()
            if v == 256:
                break
            if v > 256:
                i = v - 257
                base, xb = (3 + i, 0) if i < 8 else (258, 0) if i == 28 else (3 + ((4 + (i & 3)) << ((i >> 2) - 1)), (i >> 2) - 1)
                out.append(base + take(xb))
                ds = dist()
                take(0 if ds < 4 else (ds >> 1) - 1)
        if final:
            return out


# ---- the code builder alone ----------------------------------------------------------------------------------------------------------
def _package_merge_cost(hist, limit):
    """the optimal cost of a prefix code with lengths <= limit (boundary package-merge, plainly)"""
    w = sorted(h for h in hist if h)
    if len(w) < 2:
        return sum(w)
    packages = []
    for _ in range(limit):
        merged = sorted([(x, 1) for x in w] + packages)
        packages = [(merged[i][0] + merged[i + 1][0], 0) for i in range(0, len(merged) - 1, 2)]
        last = merged
    return sum(x for x, _ in last[:2 * len(w) - 2])


def _histograms(nsym):
    fib = [1, 1]
    while len(fib) < nsym:
        fib.append(min(fib[-1] + fib[-2], 60000))
    yield "fibonacci", fib[:nsym]
    yield "one", [0] * (nsym - 1) + [7]
    yield "one_first", [9] + [0] * (nsym - 1)
    yield "two", [0, 5] + [0] * (nsym - 3) + [1]
    yield "equal", [3] * nsym
    yield "huge_and_ones", [50000] + [1] * (nsym - 1)
    g = D._lcg(nsym)
    yield "random", [next(g) % 1000 if next(g) % 3 else 0 for _ in range(nsym)]


@pytest.mark.parametrize("nsym,limit,pad", [(286, 15, 0), (30, 15, 0), (19, 7, 1)])
def test_code_builder(nsym, limit, pad):
    L = E.lib()
    for name, hist in _histograms(nsym):
        h = (C.c_uint32 * nsym)(*hist)
        got, want = (C.c_ubyte * nsym)(), (C.c_ubyte * nsym)()
        assert L.sim_dfe_build_lens(h, nsym, limit, pad, got) != E.SIM_BOUNDS, name
        L.dfe_model_build_lens(h, nsym, limit, pad, want)
        lens = list(got)
        assert lens == list(want), name
        used = [s for s in range(nsym) if hist[s]]
        coded = [s for s in range(nsym) if lens[s]]
        assert set(used) <= set(coded) and (coded == used or (pad and len(used) == 1 and len(coded) == 2)), name
        kraft = sum(2.0 ** -lens[s] for s in coded)
        assert kraft <= 1.0 and max(lens) <= limit, (name, kraft, max(lens))
        if len(coded) >= 2:
            assert kraft == 1.0, (name, kraft)
        else:
            assert lens[used[0]] == 1
        # canonical order: by (length, symbol), each code the successor of the one before, shifted at a length's start
        codes = (C.c_uint32 * nsym)()
        assert L.sim_dfe_assign_codes(got, nsym, limit, codes) != E.SIM_BOUNDS, name
        code, prev = 0, 0
        for ln, s in sorted((lens[s], s) for s in coded):
            code <<= ln - prev
            prev = ln
            assert codes[s] >> 16 == ln and int(format(codes[s] & 0xffff, "0%db" % ln)[::-1], 2) == code, (name, s)
            code += 1
        cost = sum(hist[s] * lens[s] for s in used)
        best = _package_merge_cost(hist, limit)
        print("%-14s nsym %3d limit %2d: cost %8d optimal %8d excess %.4f %%" % (name, nsym, limit, cost, best, 100.0 * (cost - best) / max(best, 1)))
        assert cost >= best


# ---- the ratio over the corpus, on the model ----------------------------------------------------------------------------------------------
# bytes of this encoder / bytes of zlib level 1 (raw, per 64 KiB chunk), per file, rounded up to the next whole percent
PINNED = {"Mark.Twain-Tom.Sawyer.txt": 1.00, "alice29.txt": 0.99, "asyoulik.txt": 0.98, "dickens.sample64k": 0.99, "fireworks.jpeg": 1.01,
          "geo.protodata": 0.98, "html": 1.02, "html_x_4": 1.01, "kppkn.gtb": 1.04, "lcet10.txt": 0.98, "mr.sample64k": 1.04,
          "nci.sample64k": 0.93, "ooffice.sample64k": 1.07, "osdb.sample64k": 1.00, "paper-100k.pdf": 1.01, "plrabn12.txt": 0.98,
          "reymont.sample64k": 1.04, "urls.10K": 1.01, "x-ray.sample64k": 1.08, "xml.sample64k": 0.96}


def test_ratio_over_the_corpus():
    from test_enc2_model import model_lib, model_lz4
    lz4 = model_lib()
    total = total_zlib = total_lz4 = 0
    seen = set()
    for f in E.corpus_files():
        name = os.path.basename(f)[:-4]
        a = z = l4 = 0
        for c in E.corpus_chunks(f):
            a += E.model(c, E.RAW)[0]
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            z += len(co.compress(c) + co.flush())
            l4 += len(model_lz4(lz4, c))
        print("%-28s this %8d zlib-1 %8d ratio %.4f lz4 model %8d" % (name, a, z, a / z, l4))
        assert a <= PINNED[name] * z, (name, a / z)
        seen.add(name)
        total += a; total_zlib += z; total_lz4 += l4
    print("total: this %d zlib-1 %d (%.4f) lz4 model %d" % (total, total_zlib, total / total_zlib, total_lz4))
    assert seen == set(PINNED)
    assert total <= 1.05 * total_zlib and total < total_lz4
