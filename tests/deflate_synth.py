"""DEFLATE streams that no compressor writes, for tests/test_deflate_synth_model.py and tests/test_deflate_synth_gpu.py: a seeded,
deterministic synthesizer on the bit writer of tests/deflate_cases.py.  Every case is Case(name, wrap, stream, expected, features,
cuts): `expected` are the bytes the stream decodes to by the generator's OWN bookkeeping (None: a stream built to be refused, only
family `headers`' hclen_4), `features` the names of what the case was built to contain, `cuts` further capacities at which the tests
decode it (a literal run cut at 62..65 literals, a stored block cut at its edges).  Families (cases() builds all of them once):

    codes          dynamic blocks over random complete codes: deepest (1, 2, ..., 14, 15, 15), flat, skewed, uniform-random and chains
                   to every depth behind the 9-bit and 6-bit roots; 1 .. 256 literals, all 286 symbols; 0 .. 30 distance symbols
    headers        code lengths sent plain and run-length coded: runs that cross from the literal/length lengths into the distance
                   lengths, the longest run, a repeat of a zero, short and deep code-length codes, HLIT 257, HDIST 1
    matches        every (distance, length) of GRID_DISTANCES x GRID_LENGTHS in fixed and dynamic blocks, length 258 as symbol 284 + 31,
                   every length and distance symbol at its first and last value, matches that read literals of their own round
    literal_runs   runs of RUNS literals from the start of a round, ended by a match, an end of block or the end of the stream (and,
                   through `cuts`, by the capacity)
    stored         stored blocks of STORED_LENGTHS at each of the 8 bit offsets, a Huffman block behind whose first match reads the
                   stored bytes; two and three stored blocks back to back
    blocks         1, 2 and 40 blocks in every order of types; empty fixed / dynamic blocks, a final empty stored block
    wrappers       all of them raw; a seeded third also as zlib (CINFO 0 / 7) and gzip (FEXTRA of 0, 253..260, 65 535 bytes, FNAME and
                   FCOMMENT of 300 bytes, FHCRC on and off)

hclen_4: with only the first four code-length-code lengths sent (symbols 16, 17, 18 and 0) every code length is 0, the end-of-block
code is missing and inflate refuses the block, so those cases are refusals by construction; hclen_5 (16, 17, 18, 0, 8: 256 codes of 8
bits) is the shortest code-length code of a stream inflate accepts.  Data and helpers only: no GPU, no compressor."""
import random
import zlib
from collections import namedtuple

import deflate_cases as D

Case = namedtuple("Case", "name wrap stream expected features cuts")

GRID_DISTANCES = tuple(range(1, 67)) + (127, 128, 129, 130, 255, 256, 257, 258, 32767, 32768)
GRID_LENGTHS = (3, 4, 63, 64, 65, 66, 127, 128, 129, 257, 258)
RUNS = (1, 63, 64, 65, 127, 128, 129)
RUN_CUTS = (62, 63, 64, 65)
STORED_LENGTHS = (0, 1, 3, 4, 5) + tuple(range(251, 261)) + tuple(range(500, 513)) + (1023, 1024, 1025, 65535)
# the features every family must produce in at least three cases (tests/test_deflate_synth_model.py asserts it)
LISTED = (["lit_len_15", "dist_len_15", "all_286", "all_30", "one_distance_code", "no_distance_code"]
          + ["lit_subtable_width_%d" % k for k in range(1, 7)] + ["dist_subtable_width_%d" % k for k in range(1, 10)]
          + ["run16_crosses_alphabets", "run17_crosses_alphabets", "run18_crosses_alphabets", "run18_138", "run16_after_zero", "hclen_4",
             "cl_code_len_7", "hlit_257", "hdist_1"]
          + ["len258_as_284_31", "max_extra_bits", "match_reads_the_literals_of_its_own_round", "distance_32768"])

LEN_EXTRA = [0] * 8 + [k for k in range(1, 6) for _ in range(4)] + [0]
LEN_BASE = [3 + sum(1 << LEN_EXTRA[j] for j in range(i)) for i in range(28)] + [258]
DIST_EXTRA = [0, 0] + [k for k in range(0, 14) for _ in range(2)]
DIST_BASE = [1 + sum(1 << DIST_EXTRA[j] for j in range(i)) for i in range(30)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_symbol(n):
    return 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)


def dist_symbol(d):
    return max(i for i in range(30) if DIST_BASE[i] <= d)


class Writer:
    """deflate_cases.Bits with an integer behind it (the same calls: put, code, align, raw, bytes), for streams of many kilobytes"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 256:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k
        return self

    def code(self, c, n):
        return self.put(int(format(c, "0%db" % n)[::-1], 2), n)

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        return self.put(0, -self.n % 8)

    def raw(self, data):
        self.align()
        self.out += self.acc.to_bytes(self.n >> 3, "little") + bytes(data)
        self.acc = self.n = 0
        return self

    def bytes(self):
        return bytes(self.out + self.acc.to_bytes((self.n + 7) >> 3, "little"))


def enc_table(lens):
    """symbol -> (code with its bits reversed, length): what Writer.put takes"""
    return {s: (int(format(c, "0%db" % n)[::-1], 2), n) for s, (c, n) in D.canon(lens).items()}


# ---- complete codes -------------------------------------------------------------------------------------------------------------------
def shape_lengths(n, shape, rng, maxlen=15):
    """the lengths of a complete code of n >= 2 symbols (n == 1: one code of one bit; 0: none), in no particular order.  A leaf of length
    l split into two of l + 1 keeps the code complete: `deepest` starts from the chain 1, 2, ..., m, m down to maxlen, `chainK` from the
    chain down to K and never goes deeper, `flat` splits the shortest leaf, `skewed` the longer of two random leaves, `random` any."""
    if n <= 1:
        return [1] * n
    depth = maxlen
    if shape.startswith("chain"):
        depth = int(shape[5:])
    if shape == "deepest" or shape.startswith("chain"):
        m = min(depth, n - 1)
        lens = list(range(1, m + 1)) + [m]
    else:
        lens = [1, 1]
    while len(lens) < n:
        ok = [i for i, l in enumerate(lens) if l < depth]
        if shape == "flat":
            i = min(ok, key=lambda i: lens[i])
        elif shape == "skewed":
            i = max(rng.choice(ok), rng.choice(ok), key=lambda i: lens[i])
        else:
            i = rng.choice(ok)
        lens[i] += 1
        lens.append(lens[i])
    assert sum(1 << (15 - l) for l in lens) == 1 << 15 and max(lens) <= maxlen
    return lens


def assign(symbols, lens, rng, nsym):
    """the code lengths of an alphabet of nsym symbols: the given lengths dealt to the given symbols in a random order"""
    lens = list(lens)
    rng.shuffle(lens)
    out = [0] * nsym
    for s, l in zip(symbols, lens):
        out[s] = l
    return out


def subtable_widths(lens, root):
    """the widths of the sub-tables a two-level table of this root has: per root prefix the longest code below it, less the root"""
    widths = {}
    for s, (c, n) in D.canon(lens).items():
        if n > root:
            p = c >> (n - root)
            widths[p] = max(widths.get(p, 0), n - root)
    return set(widths.values())


def table_features(litlens, distlens):
    f = set()
    if 15 in litlens:
        f.add("lit_len_15")
    if 15 in distlens:
        f.add("dist_len_15")
    f |= {"lit_subtable_width_%d" % k for k in subtable_widths(litlens, 9)}
    f |= {"dist_subtable_width_%d" % k for k in subtable_widths(distlens, 6)}
    if len(litlens) == 286 and all(litlens):
        f.add("all_286")
    if len(distlens) == 30 and all(distlens):
        f.add("all_30")
    used = sum(1 for l in distlens if l)
    if used == 1:
        f.add("one_distance_code")
    if used == 0:
        f.add("no_distance_code")
    if len(litlens) == 257:
        f.add("hlit_257")
    if len(distlens) == 1:
        f.add("hdist_1")
    return f


# ---- the code lengths of a dynamic header ---------------------------------------------------------------------------------------------
def rle(seq, mode):
    """[(symbol, extra bits value, first index, count)] of the code-length symbols that send seq.  plain: every length as itself;
    greedy: 18 / 17 for runs of zeros (18 up to 138), 16 for repeats, over the whole sequence — a run never stops at the border between
    the two alphabets; zero16: runs of zeros as a 0 and 16s that repeat it"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if mode == "plain":
            out += [(v, 0, i + k, 1) for k in range(run)]
            i = j
            continue
        if v == 0 and mode != "zero16":
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, i, r)); i += r; run -= r
            if run >= 3:
                out.append((17, run - 3, i, run)); i += run; run = 0
        else:
            out.append((v, 0, i, 1)); i += 1; run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, i, r)); i += r; run -= r
        out += [(v, 0, i + k, 1) for k in range(run)]
        i = j
    return out


def header_features(events, seq, nlen):
    f = set()
    for s, x, at, cnt in events:
        if s >= 16 and at < nlen < at + cnt:
            f.add("run%d_crosses_alphabets" % s)
        if s == 18 and cnt == 138:
            f.add("run18_138")
        if s == 16 and seq[at - 1] == 0:
            f.add("run16_after_zero")
    return f


def cl_code(used, shape, rng):
    """the 19 lengths of a complete code-length code over the symbols in use (inflate refuses an incomplete one, a single code included:
    a second symbol joins a lone one)"""
    used = sorted(used)
    if len(used) < 2:
        used.append(next(s for s in (1, 2, 0) if s not in used))
    return assign(used, shape_lengths(len(used), shape, rng, 7), rng, 19)


class Synth:
    """one stream in the making: the blocks written so far, the bytes they decode to and what they were built to contain"""

    def __init__(self, seed=0):
        self.w, self.out, self.features, self.rng, self.max_dist = Writer(), bytearray(), set(), random.Random(seed), 0
        self.accepted = True

    def _ops(self, ops, lit, dist):
        w, out = self.w, self.out
        for op in ops:
            if isinstance(op, int):
                w.put(*lit[op])
                out.append(op)
                continue
            n, d = op[0], op[1]
            ls = 27 if len(op) > 2 else len_symbol(n)                        # (n, d, "284"): length 258 as symbol 284 with extra bits 31
            w.put(*lit[257 + ls]).put(n - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = dist_symbol(d)
            w.put(*dist[ds]).put(d - DIST_BASE[ds], DIST_EXTRA[ds])
            assert 1 <= d <= len(out) and d <= 32768 and 3 <= n <= 258, (n, d, len(out))
            self.max_dist = max(self.max_dist, d)
            if d == 32768:
                self.features.add("distance_32768")
            if len(op) > 2:
                self.features.add("len258_as_284_31")
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
        w.put(*lit[256])

    def stored(self, data, final=0):
        self.w.put(final, 1).put(0, 2).align().put(len(data), 16).put(len(data) ^ 0xFFFF, 16).raw(data)
        self.out += data
        return self

    def fixed(self, ops, final=0):
        self.w.put(final, 1).put(1, 2)
        self._ops(ops, enc_table(FIXED_LIT), enc_table(FIXED_DIST))
        return self

    def dynamic(self, ops, litlens, distlens, final=0, mode="greedy", cl_shape="flat", ncode=None, cl_lens=None):
        """a dynamic block over the given code lengths (lists of HLIT and HDIST entries); mode: rle()'s; cl_shape: the code-length code's
        shape (shape_lengths, at most 7 bits); ncode: how many of its lengths are sent (None: up to the last one in use)"""
        seq = list(litlens) + list(distlens)
        events = rle(seq, mode)
        if cl_lens is None:
            cl_lens = cl_code({e[0] for e in events}, cl_shape, self.rng)
        if ncode is None:
            ncode = max(4, 1 + max(k for k, s in enumerate(D.CL_ORDER) if cl_lens[s]))
        self.features |= table_features(litlens, distlens) | header_features(events, seq, len(litlens))
        if 7 in cl_lens:
            self.features.add("cl_code_len_7")
        if ncode in (4, 5):
            self.features.add("hclen_%d" % ncode)
        D.dyn_header(self.w, litlens, distlens, final, [(s, x) for s, x, _, _ in events], cl_lens=cl_lens, ncode=ncode)
        self._ops(ops, enc_table(litlens), enc_table(distlens))
        return self

    def auto(self, ops, final=0, shape="random", **kw):
        """a dynamic block over a random complete code of exactly the symbols that ops use"""
        lits = sorted({op for op in ops if isinstance(op, int)} | {256} | {257 + (27 if len(op) > 2 else len_symbol(op[0])) for op in ops if not isinstance(op, int)})
        dists = sorted({dist_symbol(op[1]) for op in ops if not isinstance(op, int)})
        litlens = assign(lits, shape_lengths(len(lits), shape, self.rng), self.rng, max(257, lits[-1] + 1))
        distlens = assign(dists, shape_lengths(len(dists), shape, self.rng), self.rng, dists[-1] + 1 if dists else 1)
        return self.dynamic(ops, litlens, distlens, final, **kw)

    def block(self, kind, ops, final=0):
        return self.fixed(ops, final) if kind == "fixed" else self.auto(ops, final)

    def case(self, name, family, cuts=()):
        window = {"fits_window_256"} if self.max_dist <= 256 else set()
        return Case(name, D.RAW, self.w.bytes(), bytes(self.out) if self.accepted else None, frozenset(self.features | window | {family}),
                    tuple(sorted({c for c in cuts if c >= 0})))


def _noise(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


# ---- the families -------------------------------------------------------------------------------------------------------------------
def family_codes():
    out = []

    def one(name, seed, shape_l, nlit, shape_d, ndist, nlens=None):
        s = Synth(seed)
        rng = s.rng
        lits = list(range(256)) if nlit == 256 else sorted(rng.sample(range(256), nlit))
        lsyms = [] if ndist == 0 else list(range(29)) if nlens is None and nlit == 256 and ndist == 30 else sorted(rng.sample(range(29), nlens or rng.choice((1, 3, 8))))
        dsyms = list(range(ndist)) if rng.random() < 0.7 or ndist >= 16 else sorted(rng.sample(range(16), ndist))
        lsymbols = lits + [256] + [257 + k for k in lsyms]
        litlens = assign(lsymbols, shape_lengths(len(lsymbols), shape_l, rng), rng, max(257, lsymbols[-1] + 1))
        distlens = assign(dsyms, shape_lengths(len(dsyms), shape_d, rng), rng, dsyms[-1] + 1 if dsyms else 1)
        reach = max([DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1 for k in dsyms] or [0])
        if reach:
            s.stored(_noise(rng, reach))                                       # enough output for every distance symbol in use
        ops = list(lits) * (2 if nlit < 100 else 1)
        rng.shuffle(ops)
        pairs = max(len(lsyms), len(dsyms))
        for k in range(pairs):                                               # every length and every distance symbol at least once
            ls, ds = lsyms[k % len(lsyms)], dsyms[k % len(dsyms)]
            m = (LEN_BASE[ls] + rng.randrange(1 << LEN_EXTRA[ls]), DIST_BASE[ds] + rng.randrange(1 << DIST_EXTRA[ds]))
            ops.insert(rng.randrange(len(ops) + 1), (min(m[0], 257) if ls == 27 else m[0], m[1]))
        s.dynamic(ops, litlens, distlens, 1, mode=rng.choice(("plain", "greedy")), cl_shape=rng.choice(("flat", "random")))
        out.append(s.case(name, "codes"))

    seed = 1000
    for shape in ("deepest", "flat", "skewed", "random"):
        for nlit in (1, 2, 3, 17, 100, 256):
            for ndist in (0, 1, 2, 5, 16, 30):
                seed += 1
                one("codes_%s_%dlit_%ddist" % (shape, nlit, ndist), seed, shape, nlit, shape, ndist)
        for k in range(3):
            seed += 1
            one("codes_%s_all286_all30_%d" % (shape, k), seed, shape, 256, ("deepest", "flat", "random")[k], 30)
    # a chain down to root + k and nothing deeper: one sub-table of width k, on purpose
    for k in range(1, 7):
        for j, nlit in enumerate((17, 100, 256)):
            seed += 1
            one("codes_lit_chain%d_%d" % (9 + k, j), seed, "chain%d" % (9 + k), nlit, "flat", (2, 5, 16)[j], nlens=8)
            assert "lit_subtable_width_%d" % k in out[-1].features
    for k in range(1, 10):
        for j, ndist in enumerate((16, 30, 16)):
            seed += 1
            one("codes_dist_chain%d_%d" % (6 + k, j), seed, "random", (17, 3, 100)[j], "chain%d" % (6 + k), ndist)
            assert "dist_subtable_width_%d" % k in out[-1].features
    return out


def family_headers():
    out = []

    def done(s, name, *must):
        c = s.case(name, "headers")
        assert set(must) <= c.features, (name, must, sorted(c.features))
        out.append(c)

    for k in range(1, 6):
        # 16 literal/length codes and 16 distance codes of 4 bits: the run of 4s from the end-of-block code on crosses the border
        s = Synth(2000 + k)
        lits = sorted(s.rng.sample(range(32, 250), 15 - k))
        litlens = assign(lits + [256] + [257 + j for j in range(k)], [4] * 16, s.rng, 257 + k)
        ops = lits + [(3 + j, 1 + j) for j in range(k)] + lits[:3] + [(3, 16)]
        done(s.dynamic(ops, litlens, [4] * 16, 1), "headers_run16_crosses_%d" % k, "run16_crosses_alphabets")
    for k, (z, y) in enumerate(((1, 2), (2, 2), (2, 6), (1, 9), (5, 8), (20, 20), (3, 8), (28, 28), (6, 5))):
        # z lengths of zero end the literal/length alphabet and y begin the distance alphabet: z + y < 11 is a 17, otherwise an 18
        s = Synth(2100 + k)
        lits = sorted(s.rng.sample(range(256), 6))
        nlen, lsym = 258 + z, 257
        litlens = assign(lits + [256, lsym], shape_lengths(8, "random", s.rng), s.rng, nlen)
        ln = LEN_BASE[lsym - 257]
        done(s.stored(_noise(s.rng, DIST_BASE[y + 1])).dynamic(lits + [(ln, DIST_BASE[y]), (ln, DIST_BASE[y + 1])] + lits, litlens, [0] * y + [1, 1], 1),
             "headers_zero_run_%d_%d" % (z, y), "run17_crosses_alphabets" if z + y < 11 else "run18_crosses_alphabets")
    for k in range(3):
        # literals from 200 on only: 200 lengths of zero in front are an 18 of 138 and one more
        s = Synth(2200 + k)
        lits = sorted(s.rng.sample(range(200, 256), 5 + k))
        litlens = assign(lits + [256, 257], shape_lengths(len(lits) + 2, "flat", s.rng), s.rng, 258)
        done(s.dynamic(lits * 3 + [(3, 2 if k else 1)], litlens, [0, 1] if k else [1], 1), "headers_run18_138_%d" % k, "run18_138")
    for k in range(3):
        s = Synth(2300 + k)
        lits = sorted(s.rng.sample(range(40, 256, 7), 6))                      # runs of 6 zeros between them: a 0 and a 16 of 5
        litlens = assign(lits + [256, 258], shape_lengths(8, "skewed", s.rng), s.rng, 259)
        done(s.dynamic(lits + [(4, 5)] + lits, litlens, [0, 0, 0, 0, 1], 1, mode="zero16"), "headers_run16_after_zero_%d" % k, "run16_after_zero")
    for k in range(3):
        # sixteen lengths and more in use and a code-length code that is a chain down to 7 bits
        s = Synth(2400 + k)
        lits = sorted(s.rng.sample(range(256), 40))
        litlens = assign(lits + [256, 257, 260], shape_lengths(43, "deepest", s.rng), s.rng, 261)
        done(s.dynamic(lits + [(3, 1), (6, 2)] + lits, litlens, [1, 1], 1, cl_shape="chain7"), "headers_cl_code_len_7_%d" % k, "cl_code_len_7")
    for k in range(3):
        # 256 codes of 8 bits and no distance code: only code-length symbols 8 and 0 (and, run-length coded, 16) are needed
        s = Synth(2500 + k)
        zero = 255 - 50 * k
        litlens = [8] * 257
        litlens[zero] = 0
        ops = [b for b in _noise(s.rng, 300) if b != zero]
        mode = ("plain", "greedy", "greedy")[k]
        cl = [0] * 19
        for sym, ln in ((0, 1), (8, 1)) if mode == "plain" else ((8, 1), (16, 2), (0, 2)):
            cl[sym] = ln
        done(s.dynamic(ops, litlens, [0], 1, mode=mode, cl_lens=cl), "headers_hclen_5_%d" % k, "hclen_5", "hlit_257", "hdist_1", "no_distance_code")
    for k in range(3):
        # only 16, 17, 18 and 0 can be sent: no end-of-block code, a refusal by construction (the header's own docstring)
        s = Synth(2600 + k)
        s.accepted = False
        cl = [0] * 19
        cl[0], cl[18 - (k & 1)] = 1, 1
        s.features.add("hclen_4")
        syms = ([(18, 127), (18, 109)], [(17, 7)] * 25 + [(17, 5)], [(0, 0)] * 258)[k]                # 258 lengths of zero
        D.dyn_header(s.w, [0] * 257, [0], 1, syms, cl_lens=cl, ncode=4)
        s.w.put(0, 64)
        out.append(s.case("headers_hclen_4_%d" % k, "headers"))
    for k in range(3):
        s = Synth(2700 + k)
        lits = sorted(s.rng.sample(range(256), 2 + 30 * k))
        litlens = assign(lits + [256], shape_lengths(len(lits) + 1, "random", s.rng), s.rng, 257)
        done(s.fixed([65, 66, (5, 2)]).dynamic(lits * 2, litlens, [0], 1, mode="plain"), "headers_hlit_257_hdist_1_%d" % k, "hlit_257", "hdist_1")
    return out


def family_matches():
    out = []
    groups = [GRID_DISTANCES[k:k + 8] for k in range(0, 80, 8) if GRID_DISTANCES[k:k + 8]]
    assert sum(len(g) for g in groups) == len(GRID_DISTANCES)
    for g, ds in enumerate(groups):
        for kind in ("fixed", "dynamic"):
            s = Synth(3000 + g)
            rng = s.rng
            if max(ds) > 258:
                s.stored(_noise(rng, 32768))
            ops = list(_noise(rng, 258 if max(ds) <= 258 else 5))
            for d in ds:
                for n in GRID_LENGTHS:
                    ops += [(n, d)] + list(_noise(rng, rng.choice((0, 1, 2, 5))))
                    s.features.add("pair_%d_%d" % (d, n))
            out.append(s.block(kind, ops, 1).case("matches_grid%d_%s" % (g, kind), "matches"))
    for k, kind in enumerate(("fixed", "dynamic", "dynamic")):
        s = Synth(3100 + k)
        ops = list(_noise(s.rng, 40 + k)) + [(258, 1 + 7 * k, "284"), 33, (258, 41 + k, "284"), (258, 300, "284")]
        out.append(s.block(kind, ops, 1).case("matches_len258_as_284_%d" % k, "matches"))
        # every length and distance symbol at its first and its last value
        s = Synth(3110 + k)
        s.stored(_noise(s.rng, 32768))
        ops = [7, 8, 9]
        for j in range(30):
            ls = j % 29
            far = DIST_BASE[j] + (1 << DIST_EXTRA[j]) - 1
            ops += [(LEN_BASE[ls], DIST_BASE[j]), j, (258, far, "284") if ls == 27 else (LEN_BASE[ls] + (1 << LEN_EXTRA[ls]) - 1, far)]
        s.features.add("max_extra_bits")
        out.append(s.block(kind, ops, 1).case("matches_max_extra_bits_%d" % k, "matches"))
        # a match behind k literals that the lanes still hold, reaching into them
        s = Synth(3120 + k)
        ops = []
        for held in (1, 2, 5, 31, 62, 63, 64, 65, 70):
            for d in sorted({1, held, held - 1, held // 2, held % 64}):
                if 1 <= d <= (held if held < 64 else held % 64):
                    ops += list(_noise(s.rng, held)) + [(3 + (d + held) % 8 * 32, d)]
        s.features.add("match_reads_the_literals_of_its_own_round")
        out.append(s.block(kind, ops, 1).case("matches_own_round_%d" % k, "matches"))
    return out


def family_literal_runs():
    out = []
    k = 0
    for run in RUNS:
        for ending in ("match", "end_of_block", "end_of_stream"):
            for prelude in (0, 1):
                k += 1
                s = Synth(4000 + k)
                kind = ("fixed", "dynamic")[(k + prelude) & 1]
                ops = [1, 2, 3, (4, 2)] * prelude                          # the run begins a round: at the block's start or behind a match
                start = 7 * prelude
                ops += list(_noise(s.rng, run))
                if ending == "match":
                    ops += [(3 + run % 7, 1 + run % 3 if run > 2 else 1)]
                s.block(kind, ops, 1 if ending != "end_of_block" else 0)
                if ending == "end_of_block":
                    s.fixed([9, 8, (3, 2)], 1)
                s.features |= {"literal_run_%d_ended_by_%s" % (run, ending), "literal_run_%d_ended_by_capacity" % run}
                out.append(s.case("literal_run_%d_%s_%d" % (run, ending, prelude), "literal_runs", [start + c for c in RUN_CUTS if c <= run + 1]))
    return out


def family_stored():
    out = []
    k = 0

    def front(s, bit):
        # a fixed block's header and end-of-block code are 10 bits: behind `bit` + 6 (mod 8) literals of 9 bits the next block begins
        # at bit offset `bit`
        nine = (bit + 6) % 8
        ops = [65 + k % 7, 66, 67] + [200 + j for j in range(nine)]
        s.fixed(ops)
        assert s.w.bitpos() % 8 == bit
        return len(ops)

    for n in STORED_LENGTHS:
        for bit in range(8):
            k += 1
            s = Synth(5000 + k)
            at = front(s, bit)
            s.stored(_noise(s.rng, n))
            reach = min(n + 2, 32768) if n else 2                           # the first match behind it reads the stored bytes (or, behind none, the literals)
            s.block(("fixed", "dynamic")[k & 1], [(3 + k % 64, 1 + (k * 7) % reach), 90, (258, reach)], 1)
            s.features.add("stored_%d_at_bit_%d" % (n, bit))
            out.append(s.case("stored_%d_bit%d" % (n, bit), "stored", [at + c for c in (0, 1, 2)] + [at + n - c for c in (0, 1, 2)]))
    for j, lens in enumerate(((255, 256), (256, 248, 8), (504, 1, 3), (0, 0, 5), (1, 0), (503, 505), (65535, 4000), (4, 252, 256))):
        k += 1
        s = Synth(5000 + k)
        at = front(s, j % 8)
        cuts = []
        for n in lens:
            s.stored(_noise(s.rng, n))
            cuts += [at, at + 1, at + n - 1, at + n]
            at += n
        s.block(("fixed", "dynamic")[k & 1], [(200, min(at, 300)), 1, 2], 1)
        s.features.add("stored_back_to_back_%d" % len(lens))
        out.append(s.case("stored_back_to_back_%s" % "_".join(map(str, lens)), "stored", cuts))
    return out


def family_blocks():
    out = []

    def add_block(s, t, final, empty=False):
        rng = s.rng
        have = len(s.out)
        ops = [] if empty else list(_noise(rng, rng.randrange(1, 9))) + ([(rng.randrange(3, 40), rng.randrange(1, min(have, 600) + 1))] if have else []) + list(_noise(rng, rng.randrange(0, 70)))
        if t == "s":
            s.stored(b"" if empty else _noise(rng, rng.randrange(1, 300)), final)
        elif t == "f":
            s.fixed(ops, final)
        else:
            s.auto(ops, final, shape=rng.choice(("random", "skewed", "flat")))

    k = 0
    orders = [a for a in "sfd"] + [a + b for a in "sfd" for b in "sfd"]
    for order in orders:
        k += 1
        s = Synth(6000 + k)
        for j, t in enumerate(order):
            add_block(s, t, j == len(order) - 1)
        out.append(s.case("blocks_%s" % order, "blocks"))
    for j in range(3):
        k += 1
        s = Synth(6000 + k)
        order = [a for a in "sfd" for b in "sfd" for _ in (0, 1)] + ["sfd"[s.rng.randrange(3)] for _ in range(22)]
        s.rng.shuffle(order)
        order = "".join(order)
        for i, t in enumerate(order):
            add_block(s, t, i == 39)
        s.features.add("blocks_40")
        out.append(s.case("blocks_40_%d" % j, "blocks"))
    for name, order in (("empty_fixed", "dFs"), ("empty_dynamic", "fDd"), ("final_empty_stored", "fdS"), ("only_empty_fixed", "F"), ("only_empty_dynamic", "D"),
                        ("only_empty_stored", "S"), ("empties", "FDSDFS")):
        k += 1
        s = Synth(6000 + k)
        for i, t in enumerate(order):
            add_block(s, t.lower(), i == len(order) - 1, t.isupper())
        s.features.add(name)
        out.append(s.case("blocks_%s" % name, "blocks"))
    return out


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------
FEXTRA = (0, 253, 254, 255, 256, 257, 258, 259, 260, 65535)


def as_zlib(c, cinfo):
    cmf = 8 | cinfo << 4
    head = bytes([cmf, (31 - (cmf << 8) % 31) % 31])
    tail = zlib.adler32(c.expected).to_bytes(4, "big") if c.expected is not None else b""
    return Case("%s_zlib%d" % (c.name, cinfo), D.ZLIB, head + c.stream + tail, c.expected, c.features | {"zlib_cinfo_%d" % cinfo}, c.cuts)


def as_gzip(c, k, rng):
    """header variant k: FEXTRA of FEXTRA[k % 10] bytes (k % 11 == 10: none), FNAME / FCOMMENT of 300 bytes, FHCRC"""
    extra = None if k % 11 == 10 else FEXTRA[k % 10]
    name, comment, hcrc = k % 3 == 0, k % 4 == 1, k % 2 == 1
    flg = (4 if extra is not None else 0) | (8 if name else 0) | (16 if comment else 0) | (2 if hcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + _noise(rng, 4) + b"\x02\x03"
    if extra is not None:
        head += extra.to_bytes(2, "little") + _noise(rng, extra)
    for on in (name, comment):
        if on:
            head += bytes(1 + rng.randrange(255) for _ in range(300)) + b"\0"
    if hcrc:
        head += (zlib.crc32(head) & 0xFFFF).to_bytes(2, "little")
    tail = zlib.crc32(c.expected).to_bytes(4, "little") + (len(c.expected) & 0xFFFFFFFF).to_bytes(4, "little") if c.expected is not None else b""
    f = {"gzip_fextra_%s" % ("none" if extra is None else extra)} | ({"gzip_fname_300"} if name else set()) | ({"gzip_fcomment_300"} if comment else set()) | {"gzip_fhcrc_%s" % ("on" if hcrc else "off")}
    return Case("%s_gzip%d" % (c.name, k), D.GZIP, head + c.stream + tail, c.expected, c.features | f, c.cuts)


_cache = {}


def cases(wrap=None):
    """every case of every family: all raw, a seeded third also in a zlib wrapper and a gzip wrapper"""
    if "all" not in _cache:
        raw = family_codes() + family_headers() + family_matches() + family_literal_runs() + family_stored() + family_blocks()
        rng = random.Random(7000)
        out, k = list(raw), 0
        for c in raw:
            if rng.randrange(3) == 0:
                # a window of 256 bytes (CINFO 0) only in front of streams that stay inside it
                out.append(as_zlib(c, 0 if k & 1 and "fits_window_256" in c.features else 7))
                # the 65 535-byte FEXTRA in front of short streams only
                kk = k if FEXTRA[k % 10] < 65535 or k % 11 == 10 or len(c.stream) < 2000 else k + 1
                out.append(as_gzip(c, kk, rng))
                k += 1
        small = [c for c in raw if c.name.startswith("literal_run")]
        out += [as_gzip(small[j], 9 + 10 * j, rng) for j in range(3)]          # ... whatever the seed chose
        assert len({c.name for c in out}) == len(out)
        _cache["all"] = out
    return _cache["all"] if wrap is None else [c for c in _cache["all"] if c.wrap == wrap]


def write_cases_file(path, others=(), only=None):
    """the file a stand-alone build of tests/hostsim/sim_deflate_decode.cpp (-DSIM_MAIN) runs: every case (and every (name, wrap, stream)
    of `others`; only: these cases and not all of them) at capacities n, n + 64, n - 1, 0 and its cuts, the four misalignments in turn, and in size mode, with zlib's verdict and
    bytes.  Format: that file's.  Returns the count.
        python -c "import sys; sys.path.insert(0, 'tests'); import deflate_synth as S, deflate_cases as D; print(S.write_cases_file('cases.bin', [(o['name'], o['wrap'], o['bytes']) for o in D.others()]))"
        python -c "import sys; sys.path.insert(0, 'tests'); from hostsim_build import build_sim; build_sim('sim_deflate_decode.cpp', 'sim_main', main=True, sanitize=True)" && ./sim_main cases.bin"""
    import struct
    rows = []
    todo = [(c.wrap, c.stream, c.cuts) for c in (cases() if only is None else only)] + [(w, s, ()) for _, w, s in others]
    for k, (wrap, s, cuts) in enumerate(todo):
        n = D.verdict(wrap, s, None)[0]
        for j, cap in enumerate(([n, n + 64, max(n - 1, 0), 0] if n >= 0 else [300, 0]) + list(cuts)):
            r, raw = D.verdict(wrap, s, cap)
            rows.append(struct.pack("<5Iq", wrap, 0, len(s), cap, (k + j) % 4, r) + s + (raw if r > 0 else b""))
        rows.append(struct.pack("<5Iq", wrap, 1, len(s), 0, k % 4, D.size_verdict(wrap, s)) + s)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(rows)) + b"".join(rows))
    return len(rows)
