"""A seeded writer of Zstandard streams that libzstd's encoder never writes: FSE table descriptions in every form of the reader, the
spec's table construction, a state encoder for one state (sequences) and two interleaved states (Huffman weights), Huffman trees of a
chosen shape with direct and FSE-compressed weights, one and four streams, every literals-header format, any mix of table modes, and a
small executor of the sequences that yields the bytes a case must decode to (NOT libzstd, NOT the decoder under test).

cases() -> [Case(name, family, stream, expected, features)]; expected None: a stream that must be refused.  `features` are tags of
zstd_cases.deep_classify, a reader that shares no code with this writer.  flips(n) -> seeded single-bit flips of the cases.

A normalized-count description cannot say "one too many": the largest value a count field holds is exactly what is left.  The sum is
broken from below (one too few with the whole alphabet described) and by a zero run that passes the alphabet."""
import base64
import hashlib
import random
import struct

import zstd_cases as Z

LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
DEFAULT = {"ll": (6, [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]),
           "of": (5, [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]),
           "ml": (6, [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7)}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
ALPHABET = {"ll": 36, "of": 32, "ml": 53}
SPOIL = ("bit_long", "lits_short")
FAMILIES = ("ncount", "fse_build", "modes", "offsets", "big_codes", "huffman", "frames")


class Refused(Exception):
    pass


class TooLong(Exception):
    """an FSE-compressed tree description of 128 bytes or more: its length byte would mean direct weights"""


class Case:
    def __init__(self, name, family, stream, expected, features, room=300):
        self.name, self.family, self.stream, self.expected, self.features = name, family, bytes(stream), expected, set(features)
        self.cap = len(expected) if expected is not None else room      # the capacity the tests call exact: for a refusal, room for what precedes it


def code_of(value, base):
    return max(c for c in range(len(base)) if base[c] <= value)


# ---- FSE ---------------------------------------------------------------------------------------------------------------------------------
def write_ncount(log, counts, log_field=None, feat=None):
    """the description of `counts` (-1: less than one; the last one not 0) at accuracy `log`, as an LSB-first bit string"""
    acc, nbit = (log - 5) if log_field is None else log_field, 4
    remaining, i = (1 << log) + 1, 0

    def put(v, nb):
        nonlocal acc, nbit
        assert 0 <= v < (1 << nb)
        acc |= v << nbit
        nbit += nb
    while i < len(counts):
        c = counts[i]
        nb = remaining.bit_length()
        low = (1 << nb) - 1 - remaining
        v = c + 1
        feat = set() if feat is None else feat
        if c == -1:
            feat.add("nc:less_than_one")
        if v < low:
            put(v, nb - 1)
            feat.add("nc:short")
        elif v < (1 << (nb - 1)):
            put(v, nb)
            feat.add("nc:long_low")
        else:
            put(v + low, nb)
            feat.add("nc:long_high")
        remaining -= abs(c)
        i += 1
        if c == 0:
            z = 0
            while i + z < len(counts) and counts[i + z] == 0:
                z += 1
            for _ in range(z // 3):
                put(3, 2)
            put(z % 3, 2)
            feat.add("nc:run3chain" if z >= 3 else "nc:run%d" % z)
            if z >= 36:
                feat.add("nc:run12")
            i += z
        if remaining <= 1:
            break
    return acc.to_bytes((nbit + 7) // 8, "little")


class Table:
    """an FSE decoding table by the spec's construction: per cell its symbol, bits and base"""
    def __init__(self, log, counts):
        size = 1 << log
        self.log, self.sym, self.nbits, self.base = log, [0] * size, [], []
        high = size
        for s, c in enumerate(counts):
            if c == -1:
                high -= 1
                self.sym[high] = s
        step, pos = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(counts):
            for _ in range(max(c, 0)):
                self.sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos >= high:
                    pos = (pos + step) & (size - 1)
        nxt = [abs(c) for c in counts]
        for s in self.sym:
            x = nxt[s]
            nxt[s] += 1
            nb = log - (x.bit_length() - 1)
            self.nbits.append(nb)
            self.base.append((x << nb) - size)

    @staticmethod
    def rle(symbol):
        t = Table.__new__(Table)
        t.log, t.sym, t.nbits, t.base = 0, [symbol], [0], [0]
        return t

    def symbols(self):
        return sorted(set(self.sym))

    def cells_of(self, s):
        return [u for u, x in enumerate(self.sym) if x == s]

    def before(self, s, nxt):
        """the one state of symbol s whose range of next states covers nxt"""
        return next(u for u in self.cells_of(s) if self.base[u] <= nxt < self.base[u] + (1 << self.nbits[u]))


def states(tab, symbols, rnd):
    """walk backwards: any state for the last symbol, then the one state per symbol that leads to the next"""
    st = [rnd.choice(tab.cells_of(symbols[-1]))]
    for s in reversed(symbols[:-1]):
        st.append(tab.before(s, st[-1]))
    return st[::-1]


def norm_counts(rnd, log, used, alphabet, less_than_one=0.3, spare=3):
    """normalized counts at `log` over the symbols `used` and a few unused ones"""
    syms = set(used)
    for _ in range(spare):
        if len(syms) < (1 << log) - 1:
            syms.add(rnd.randrange(alphabet))
    syms = sorted(syms)
    assert len(syms) <= 1 << log
    counts = [0] * (syms[-1] + 1)
    for s in syms:
        counts[s] = 1
    left = (1 << log) - len(syms)
    while left:
        s = rnd.choice(syms)
        k = rnd.randint(1, max(1, left // 2)) if rnd.random() < 0.7 else left
        counts[s] += k
        left -= k
    for s in syms:
        if counts[s] == 1 and rnd.random() < less_than_one:
            counts[s] = -1
    return counts


# ---- Huffman --------------------------------------------------------------------------------------------------------------------------------
def tree_weights(rnd, hlog, nsym, keep=None):
    """a Kraft-complete multiset of nsym weights whose longest code has hlog bits (hlog + 1 <= nsym <= 1 << hlog).  keep: a weight
    that stays in the set (its one leaf of the first chain is never split; the set may then end below nsym); at hlog 12 weight 12 is
    kept, which only the implied last weight may have"""
    assert hlog + 1 <= nsym <= (1 << hlog)
    lens = list(range(1, hlog)) + [hlog, hlog]
    kept = hlog - keep if keep is not None else 0 if hlog == 12 else None
    while len(lens) < nsym:
        free = [i for i, x in enumerate(lens) if x < hlog and i != kept]
        if not free:
            break
        k = rnd.choice(free)
        lens[k] += 1
        lens.append(lens[k])
    return [hlog + 1 - x for x in lens]


class Tree:
    """weights per symbol (0: absent) -> canonical codes from the cell order"""
    def __init__(self, weights):
        self.weights = list(weights)
        while self.weights[-1] == 0:
            self.weights.pop()
        total = sum(1 << (w - 1) for w in self.weights if w)
        self.log = total.bit_length() - 1
        assert total == 1 << self.log
        self.code, cell = {}, 0
        for w, s in sorted((w, s) for s, w in enumerate(self.weights) if w):
            self.code[s] = (cell >> (w - 1), self.log + 1 - w)
            cell += 1 << (w - 1)

    @staticmethod
    def of(rnd, hlog, symbols):
        ws = tree_weights(rnd, hlog, len(symbols))
        rnd.shuffle(ws)
        weights = [0] * (max(symbols) + 1)
        for s, w in zip(sorted(symbols), ws):
            weights[s] = w
        return Tree(weights)

    def direct(self):
        w = self.weights[:-1]
        assert len(w) <= 128
        w2 = w + [0] * (len(w) & 1)
        return bytes([127 + len(w)]) + bytes((w2[k] << 4) | w2[k + 1] for k in range(0, len(w2), 2))

    def fse(self, rnd, log, counts=None, feat=None):
        """FSE-compressed weights: two interleaved states, symbol j on state j & 1; the update behind the last symbol but one over-reads"""
        w = self.weights[:-1]
        assert len(w) >= 2
        if counts is None:
            counts = norm_counts(rnd, log, w, 12, less_than_one=0.3, spare=0)
        tab = Table(log, counts)
        head = write_ncount(log, counts, feat=feat)
        lanes = [w[0::2], w[1::2]]
        st = [None, None]
        last = (len(w) - 1) & 1                                       # the lane of the last symbol: any state
        st[last] = states(tab, lanes[last], rnd)
        other = lanes[last ^ 1]
        ends = [u for u in tab.cells_of(other[-1]) if tab.nbits[u] >= 1]           # ... of the one before it: a state that still reads
        tail = rnd.choice(ends)
        chain = [tail]
        for s in reversed(other[:-1]):
            chain.append(tab.before(s, chain[-1]))
        st[last ^ 1] = chain[::-1]
        fields = [(st[0][0], log), (st[1][0], log)]
        for j in range(len(w) - 2):
            lane, k = j & 1, j >> 1
            u = st[lane][k]
            fields.append((st[lane][k + 1] - tab.base[u], tab.nbits[u]))
        body = head + Z.backward_bits(fields)
        if len(body) >= 128:
            raise TooLong
        return bytes([len(body)]) + body

    def stream(self, lits):
        return Z.backward_bits([self.code[b] for b in lits])

    def streams(self, lits, four):
        if not four:
            return self.stream(lits)
        seg = (len(lits) + 3) // 4
        parts = [self.stream(lits[k * seg:(k + 1) * seg]) for k in range(4)]
        return struct.pack("<3H", *(len(p) for p in parts[:3])) + b"".join(parts)


def fse_tree(rnd, nsym, make, log=None):
    """(symbols, tree, how) of a tree over nsym symbols (fewer where needed) whose FSE-compressed description fits its 127 bytes: the
    symbols are drawn below a lower and lower top, so that fewer weights are described, until it does.  make(symbols) -> Tree"""
    for top in (256, 200, 150, 110, 80, 60, 40, 24):
        symbols = rnd.sample(range(top), min(nsym, top))
        tree = make(symbols)
        w = tree.weights[:-1]
        lg = log or (6 if len(set(w)) > 6 or rnd.random() < 0.5 else 5)
        counts = norm_counts(rnd, lg, w, 12, spare=0)
        try:
            return symbols, tree, ("fse", lg, counts, tree.fse(rnd, lg, counts=counts))
        except TooLong:
            pass
    raise AssertionError("no description fits")


def lit_header(kind, lhl, size, csize=None):
    """kind 0 raw, 1 RLE, 2 Huffman, 3 Treeless; lhl: the two Size_Format bits"""
    if kind < 2:
        if lhl in (0, 2):                                         # one byte: the format's second bit is the size's lowest
            assert size < 32
            return bytes([(size << 3) | kind])
        if lhl == 1:
            assert size < 4096
            return struct.pack("<H", (size << 4) | (1 << 2) | kind)
        assert size < (1 << 20)
        return struct.pack("<I", (size << 4) | (3 << 2) | kind)[:3]
    nb, lh = ((10, 3), (10, 3), (14, 4), (18, 5))[lhl]
    assert size < (1 << nb) and csize < (1 << nb)
    return (kind | (lhl << 2) | (size << 4) | (csize << (4 + nb))).to_bytes(lh, "little")


def huf_lhl(rnd, four, size, csize):
    if not four:
        return 0
    return rnd.choice([k for k, nb in ((1, 10), (2, 14), (3, 18)) if size < (1 << nb) and csize < (1 << nb)])


# ---- frames, blocks and the executor ---------------------------------------------------------------------------------------------------------
class Frame:
    """writes a frame block by block and executes it: self.out is what the frame must decode to; self.bad: it must be refused"""
    def __init__(self, rnd, long_window=False):
        """long_window: the header that bytes() will be given declares a window above 16 MiB (libzstd's choice of sequence decoder)"""
        self.rnd, self.out, self.reps, self.blocks, self.bad, self.feat = rnd, bytearray(), [1, 4, 8], [], False, set()
        self.long_window = long_window
        self.tabs, self.tree, self.prev_mode = {}, None, {}

    def _add(self, kind, payload, last, size=None):
        self.blocks.append((kind, payload, len(payload) if size is None else size, last))

    def raw(self, data, last=False):
        self.out += data
        self._add(0, bytes(data), last)

    def rle(self, byte, n, last=False):
        self.out += bytes([byte]) * n
        self._add(1, bytes([byte]), last, n)

    def literals(self, spec):
        """spec: ("raw", bytes, lhl) | ("rle", byte, n, lhl) | ("huf", bytes, tree, four, how, lhl or None) | ("treeless", bytes, four, lhl or None)
        how: "direct" | ("fse", log[, counts[, the description]]) -> (section bytes, the literals)"""
        if spec[0] == "raw":
            h = lit_header(0, spec[2], len(spec[1]))
            self.feat.add("lh:raw%d" % ((h[0] >> 2) & 3))
            return h + spec[1], spec[1]
        if spec[0] == "rle":
            h = lit_header(1, spec[3], spec[2])
            self.feat.add("lh:rle%d" % ((h[0] >> 2) & 3))
            return h + bytes([spec[1]]), bytes([spec[1]]) * spec[2]
        if spec[0] == "huf":
            _, lits, tree, four, how, lhl = spec
            if how == "direct":
                desc = tree.direct()
            elif len(how) > 3:                                       # (a description made before, to know its length)
                desc = how[3]
                write_ncount(how[1], how[2], feat=self.feat)
            else:
                desc = tree.fse(self.rnd, how[1], counts=how[2] if len(how) > 2 else None, feat=self.feat)
            self.feat.add("huf:last%d" % tree.weights[-1])
            self.feat |= {"weights:direct" if how == "direct" else "weights:fse", "huf:log%d" % tree.log}
            if how != "direct":
                self.feat.add("w:log%d" % how[1])
            if len(tree.weights) == 129 and how == "direct":
                self.feat.add("huf:128direct")
            if len(tree.weights) == 256:
                self.feat.add("huf:sym255")
            if len(tree.code) in (2, 256):
                self.feat.add("huf:%dsymbols" % len(tree.code))
            body = desc + tree.streams(lits, four)
            self.tree = tree
        else:
            _, lits, four, lhl = spec
            if self.tree is None:
                self.bad = True
                body = b"\x01" * (10 if four else 1)
            else:
                body = self.tree.streams(lits, four)
        lhl = huf_lhl(self.rnd, four, len(lits), len(body)) if lhl is None else lhl
        self.feat |= {"lh:%s%d" % (spec[0] if spec[0] == "huf" else "treeless", lhl), "lit:treeless" if spec[0] == "treeless" else "lit:huf4" if four else "lit:huf1"}
        return lit_header(2 if spec[0] == "huf" else 3, lhl, len(lits), len(body)) + body, lits

    def table(self, name, mode, symbols):
        """the bytes of one table in `mode`: "predefined" | "rle" | ("fse", log[, counts]) | "repeat"; sets self.tabs[name]"""
        mname = mode if isinstance(mode, str) else mode[0]
        if name in self.prev_mode:
            self.feat.add("%s:%s>%s" % (name, self.prev_mode[name], mname))
        self.prev_mode[name] = mname
        if mname == "predefined":
            self.tabs[name] = Table(*DEFAULT[name])
            return b""
        if mname == "rle":
            assert len(set(symbols)) == 1
            self.tabs[name] = Table.rle(symbols[0])
            return bytes([symbols[0]])
        if mname == "fse":
            log = mode[1]
            counts = mode[2] if len(mode) > 2 else norm_counts(self.rnd, log, symbols, ALPHABET[name] if name != "of" else 29)
            self.tabs[name] = Table(log, counts)
            self.feat.add("%s:log%d" % (name, log))
            return write_ncount(log, counts, feat=self.feat)
        if name not in self.tabs:
            self.bad = True
            self.tabs[name] = Table.rle(symbols[0])
        return b""

    def execute(self, lits, seqs):
        at = 0
        for ll, ml, code, extra in seqs:
            if ll > len(lits) - at:
                raise Refused("literals")
            self.out += lits[at:at + ll]
            at += ll
            value = (1 << code) + extra
            if value > 3:
                self.reps = [value - 3, self.reps[0], self.reps[1]]
                self.feat.add("off:new")
            else:
                k = value - 1 + (ll == 0)
                self.feat.add(("off:rep1", "off:ll0_rep2" if ll == 0 else "off:rep2", "off:ll0_rep3" if ll == 0 else "off:rep3", "off:ll0_rep1m1")[k])
                if k:
                    t = self.reps[k] if k < 3 else self.reps[0] - 1
                    if t == 0:
                        t = 1
                        self.feat.add("off:forced1")
                    self.reps = [t, self.reps[0], self.reps[1]] if k > 1 else [t, self.reps[0], self.reps[2]]
            off = self.reps[0]
            if off > len(self.out):
                raise Refused("offset")
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                pat = bytes(self.out[-off:])
                self.out += (pat * (ml // off + 1))[:ml]
        self.out += lits[at:]

    def compressed(self, lit_spec, seqs, modes=("predefined", "predefined", "predefined"), last=False, tail=None, spoil=None):
        """a compressed block: the literals, then seqs = [(literal length, match length, offset code, offset extra bits)];
        modes: (LL, OF, ML).  spoil: a refusal by construction — "bit_long": more bits than the sequences and their last state updates read; "lits_short": raw
        literals one fewer than the sequences take; "cut_tail": the bits of the last three sequences are missing (only where libzstd's
        prefetching sequence decoder runs, which refuses the over-read; its other one reads zeros)"""
        if spoil == "lits_short" and (lit_spec[0] != "raw" or sum(s[0] for s in seqs) == 0 or len(lit_spec[1]) in (32, 4096)):
            spoil = "bit_long"
        if spoil == "lits_short":
            lit_spec = ("raw", lit_spec[1][:sum(s[0] for s in seqs) - 1], lit_spec[2])
        section, lits = self.literals(lit_spec)
        body = section + Z.nseq_bytes(len(seqs))
        if seqs:
            cl = [code_of(s[0], LL_BASE) for s in seqs]
            cm = [code_of(s[1], ML_BASE) for s in seqs]
            co = [s[2] for s in seqs]
            mbyte = 0
            for m, sh in zip(modes, (6, 4, 2)):
                mbyte |= ("predefined", "rle", "fse", "repeat").index(m if isinstance(m, str) else m[0]) << sh
            body += bytes([mbyte])
            body += self.table("ll", modes[0], cl) + self.table("of", modes[1], co) + self.table("ml", modes[2], cm)
            T = self.tabs
            for name, used in (("ll", cl), ("of", co), ("ml", cm)):
                if not set(used) <= set(T[name].sym):
                    raise ValueError("%s: code outside the table" % name)
            sl, so, sm = states(T["ll"], cl, self.rnd), states(T["of"], co, self.rnd), states(T["ml"], cm, self.rnd)
            fields = [(sl[0], T["ll"].log), (so[0], T["of"].log), (sm[0], T["ml"].log)]
            # libzstd's prefetching decoder: a window above 16 MiB, more than 4 sequences, 7 / 256 of the offset cells above 22 bits
            prefetch = self.long_window and len(seqs) > 4 and (sum(1 for x in T["of"].sym if x > 22) << (8 - T["of"].log)) >= 7
            if prefetch:
                self.feat.add("seq:prefetch")
            marks = []
            for i, s in enumerate(seqs):
                marks.append(len(fields))
                fields += [(s[3], co[i]), (s[1] - ML_BASE[cm[i]], ML_BITS[cm[i]]), (s[0] - LL_BASE[cl[i]], LL_BITS[cl[i]])]
                total = co[i] + ML_BITS[cm[i]] + LL_BITS[cl[i]]
                if total >= 31:
                    self.feat.add("seq:reload31")
                if 30 <= total <= 32:
                    self.feat.add("seq:bits%d" % total)
                if i + 1 < len(seqs):
                    for tab, st in ((T["ll"], sl), (T["ml"], sm), (T["of"], so)):
                        fields.append((st[i + 1] - tab.base[st[i]], tab.nbits[st[i]]))
            if spoil == "bit_long":
                fields.append((0, 27))                              # (the last sequence's state updates read up to 26 of them)
                if prefetch:                                         # that decoder does not ask for the stream's exact end
                    self.feat.add("seq:leftover_bits")
                else:
                    self.bad = True
            if spoil == "cut_tail":
                assert prefetch and len(seqs) > 3
                fields = fields[:marks[-3]]
                self.bad = True
            body += Z.backward_bits(fields) if tail is None else tail
        try:                                                         # (of a block that is refused too: the room its case is given)
            self.execute(lits, seqs)
        except Refused:
            self.bad = True
        self._add(2, body, last)
        return body

    def bytes(self, header=None, checksum=None, content=None):
        """header: the bytes between the magic and the first block (default: descriptor 0 or 4, window 0x58)"""
        checksum = self.rnd.random() < 0.5 if checksum is None else checksum
        if header is None:
            header = bytes([4 if checksum else 0, 0x58])
        else:
            header = bytes([header[0] | (4 if checksum else 0)]) + header[1:]
        blocks = list(self.blocks)
        if not blocks[-1][3]:
            blocks[-1] = blocks[-1][:3] + (True,)
        body = b"".join(struct.pack("<I", (size << 3) | (kind << 1) | (1 if last else 0))[:3] + payload for kind, payload, size, last in blocks)
        content = bytes(self.out) if content is None else content
        return b"\x28\xb5\x2f\xfd" + header + body + (struct.pack("<I", Z.xxh64(content) & 0xFFFFFFFF) if checksum else b"")


def random_seqs(rnd, f, nseq, ll_codes, of_codes, ml_codes):
    """nseq sequences over the given codes that are valid behind f.out (of_codes: 0 and 1 are the repeat codes); -> (seqs, literals)"""
    seqs, have, reps, nlit = [], len(f.out), list(f.reps), 0
    for _ in range(nseq):
        cl, cm = rnd.choice(ll_codes), rnd.choice(ml_codes)
        ll = LL_BASE[cl] + rnd.randrange(1 << LL_BITS[cl])
        ml = ML_BASE[cm] + rnd.randrange(1 << ML_BITS[cm])
        have += ll
        for _try in range(50):
            co = rnd.choice(of_codes)
            if co >= 2:
                lo = (1 << co) - 3
                if lo > have:
                    continue
                extra = rnd.randrange(min(1 << co, have - lo + 1))
                nreps = [lo + extra, reps[0], reps[1]]
            else:
                extra = rnd.randrange(2) if co else 0
                k = co + extra + (ll == 0)
                if k == 0:
                    nreps = reps
                else:
                    t = (reps[k] if k < 3 else reps[0] - 1) or 1
                    nreps = [t, reps[0], reps[1]] if k > 1 else [t, reps[0], reps[2]]
                if nreps[0] > have:
                    continue
            break
        else:
            raise ValueError("no offset code fits")
        reps = nreps
        have += ml
        nlit += ll
        seqs.append((ll, ml, co, extra))
    return seqs, nlit


def rnd_bytes(rnd, n, alphabet=256):
    return bytes(rnd.randrange(alphabet) for _ in range(n))


def simple_lits(rnd, n):
    return ("raw", rnd_bytes(rnd, n), 1 if n >= 32 or rnd.random() < 0.5 else rnd.choice((0, 2)))


# ---- the families ---------------------------------------------------------------------------------------------------------------------------
def _finish(out, name, family, f, feats=(), stream=None, refuse=False, **kw):
    stream = f.bytes(**kw) if stream is None else stream
    bad = f.bad or refuse
    out.append(Case(name, family, stream, None if bad else bytes(f.out), set(feats) if bad else set(feats) | f.feat, room=max(300, len(f.out) + 64)))


def _start(seed, prefix=600):
    rnd = random.Random(seed)
    f = Frame(rnd)
    if prefix:
        f.raw(rnd_bytes(rnd, prefix, 7))
    return rnd, f


def _sym_seqs(rnd, f, name, symbols, nseq):
    """sequences whose `name` codes are drawn from symbols (each at least once when nseq allows); the other two codes small"""
    pools = {"ll": [0, 1, 2, 5, 17], "of": [0, 1, 3, 5], "ml": [0, 1, 4, 33]}
    pools[name] = list(symbols)
    seqs, nlit = random_seqs(rnd, f, nseq, pools["ll"], pools["of"], pools["ml"])
    return seqs, nlit


def family_ncount(out):
    fam = "ncount"
    k = 0
    for name, idx in (("ll", 0), ("of", 1), ("ml", 2)):
        small = {"ll": list(range(0, 20)), "of": list(range(0, 9)), "ml": list(range(0, 40))}[name]
        for log in range(5, MAX_LOG[name] + 1):
            for rep in range(5):
                rnd, f = _start(1000 + k)
                k += 1
                used = rnd.sample(small, rnd.randint(1, min(len(small), 12)))
                seqs, nlit = _sym_seqs(rnd, f, name, used, rnd.randint(1, 40))
                modes = ["predefined"] * 3
                modes[idx] = ("fse", log)
                f.compressed(simple_lits(rnd, nlit + rnd.randrange(4)), seqs, tuple(modes), spoil=SPOIL[k & 1] if rep == 4 else None)
                _finish(out, "nc_%s_log%d_%d" % (name, log, rep), fam, f)
        # the accuracy log one above the maximum and 15 plus: refused
        for log, field in ((MAX_LOG[name] + 1, None), (MAX_LOG[name], 11), (MAX_LOG[name], 15)):
            rnd, f = _start(1000 + k)
            k += 1
            seqs, nlit = _sym_seqs(rnd, f, name, small[:3], 5)
            modes = ["predefined"] * 3
            counts = norm_counts(rnd, log, small[:3], 8)
            modes[idx] = ("fse", log, counts)
            f.compressed(simple_lits(rnd, nlit), seqs, tuple(modes))
            if field is not None:                                # the same description with a log field of 16 / 20
                kind, payload, size, last = f.blocks[-1]
                good = write_ncount(log, counts)
                bad = write_ncount(log, counts, log_field=field)
                assert payload.count(good) == 1
                f.blocks[-1] = (kind, payload.replace(good, bad), size, last)
            _finish(out, "nc_%s_log_too_large_%d" % (name, log if field is None else field + 5), fam, f, refuse=True)
        # only "less than one" counts; one symbol owning all but one cell
        for log in (5, 6):
            rnd, f = _start(1000 + k)
            k += 1
            if (1 << log) <= ALPHABET[name] - (3 if name == "of" else 0):
                counts = [-1] * (1 << log)
                seqs, nlit = _sym_seqs(rnd, f, name, [c for c in small if c < (1 << log)], 20)
                modes = ["predefined"] * 3
                modes[idx] = ("fse", log, counts)
                f.compressed(simple_lits(rnd, nlit), seqs, tuple(modes))
                _finish(out, "nc_%s_all_less_than_one_log%d" % (name, log), fam, f)
            rnd, f = _start(1000 + k)
            k += 1
            a, b = rnd.sample(small[:8], 2)
            counts = [0] * (max(a, b) + 1)
            counts[a], counts[b] = (1 << log) - 1, rnd.choice((1, -1))
            seqs, nlit = _sym_seqs(rnd, f, name, [a, b], 12)
            modes = ["predefined"] * 3
            modes[idx] = ("fse", log, counts)
            f.compressed(simple_lits(rnd, nlit), seqs, tuple(modes))
            _finish(out, "nc_%s_one_owns_all_but_one_log%d" % (name, log), fam, f)
        # one too few with the whole alphabet described; a zero run past the alphabet; a symbol above the alphabet
        top = ALPHABET[name] if name != "of" else 32
        for how in ("too_few", "run_past", "above"):
            rnd, f = _start(1000 + k)
            k += 1
            log = 6
            if how == "too_few":
                counts = [1] * top
                counts[0] = (1 << log) - top                      # sums to (1 << log) - 1
            elif how == "run_past":
                counts = [(1 << log) - 1, 0] + [0] * top + [1]
            else:
                counts = [(1 << log) - 1] + [0] * (top - 1) + [1]     # symbol `top`
            seqs, nlit = _sym_seqs(rnd, f, name, [0], 3)
            modes = ["predefined"] * 3
            modes[idx] = ("fse", log, counts)
            f.compressed(simple_lits(rnd, nlit), seqs, tuple(modes))
            _finish(out, "nc_%s_%s" % (name, how), fam, f, refuse=True)
    # OF symbols 29..31 described but unused
    for sym in (29, 30, 31):
        rnd, f = _start(1000 + k)
        k += 1
        counts = [10, 10, 5, 4] + [0] * (sym - 4) + [rnd.choice((3, 2))]
        counts[0] += 32 - sum(counts)
        seqs, nlit = _sym_seqs(rnd, f, "of", [0, 1, 2, 3], 10)
        f.compressed(simple_lits(rnd, nlit), seqs, ("predefined", ("fse", 5, counts), "predefined"))
        _finish(out, "nc_of_symbol_%d_unused" % sym, fam, f)
    # zero runs: flags 0 / 1 / 2, chained 3s and 12 pairs and more (ML has the room), with the symbol behind the run used
    for gap in (0, 1, 2, 3, 4, 5, 6, 8, 9, 20, 35, 36, 37, 38, 40, 44, 50):
        rnd, f = _start(1000 + k)
        k += 1
        counts = [rnd.randint(1, 20)] + [0] * (gap + 1) + [1]
        counts[-1] = 64 - counts[0]
        seqs, nlit = _sym_seqs(rnd, f, "ml", [0, gap + 2], 8)
        f.compressed(simple_lits(rnd, nlit), seqs, ("predefined", "predefined", ("fse", 6, counts)))
        _finish(out, "nc_ml_zero_run_%d" % (gap + 1), fam, f)
    # a description that is all of a block's rest but a short bitstream: under 8 bytes (the zero-padded copy), the tail path, and one
    # that ends exactly at its block's end (no bitstream: refused) or runs past it
    for rep in range(12):
        rnd, f = _start(1000 + k)
        k += 1
        n = rnd.choice((2, 3, 2, 9, 14, 20))
        used = sorted(rnd.sample(range(0, 40), n))
        counts = norm_counts(rnd, rnd.choice((5, 6, 7)) if n < 9 else 7, used, 53, spare=0)
        seqs, nlit = _sym_seqs(rnd, f, "ml", used, 1)
        seqs = [(s[0], s[1], 0, 0) for s in seqs]                 # the first repeat offset: no offset bits
        log = sum(abs(c) for c in counts).bit_length() - 1
        body = f.compressed(("raw", rnd_bytes(rnd, nlit), 0 if nlit < 32 else 1), seqs, ("rle", "rle", ("fse", log, counts)))
        desc = write_ncount(log, counts)
        rest = len(body) - body.index(desc)
        _finish(out, "nc_ml_short_rest_%d" % rep, fam, f, feats=("nc:under8",) if rest < 8 else ("nc:tail",) if len(desc) >= rest - 1 else ())
    for how in ("block_end", "past_block"):
        for rep in range(3):
            rnd, f = _start(1000 + k)
            k += 1
            used = sorted(rnd.sample(range(0, 40), 6 + rep))
            counts = norm_counts(rnd, 6, used, 53, spare=0)
            seqs, nlit = _sym_seqs(rnd, f, "ml", used, 2)
            seqs, nlit = [(3, s[1], 0, 0) for s in seqs], 6
            desc = write_ncount(6, counts)
            body = f.compressed(simple_lits(rnd, nlit), seqs, ("rle", "rle", ("fse", 6, counts)))
            at = body.index(desc) + len(desc)
            kind, payload, size, last = f.blocks[-1]
            cut = payload[:at] if how == "block_end" else payload[:at - len(desc) // 2 - 1]
            f.blocks[-1] = (kind, cut, len(cut), last)
            _finish(out, "nc_ml_%s_%d" % (how, rep), fam, f, refuse=True, feats=("nc:block_end",) if how == "block_end" else ())
    # the weights' table: every log, and at log 5 and 6 descriptions of 12, 13 and 14 symbols (symbols 11, 12 and 13 are never decoded:
    # a weight of 12 or more is refused)
    for log in (5, 6):
        for nsym in (6, 9, 11, 12, 13, 14, 91, 92, 93, 94):             # (the long zero runs take the reader's 24-bit skip)
            for rep in range(6 if nsym < 90 else 4):
                rnd, f = _start(1000 + k, prefix=0)
                k += 1
                hlog = rnd.randint(3, min(8, nsym - 1))
                symbols = rnd.sample(range(120), rnd.randint(hlog + 1, min(1 << hlog, 60)))
                tree = Tree.of(rnd, hlog, symbols)
                used = sorted(set(tree.weights[:-1]))
                counts = norm_counts(rnd, log, used, 11, spare=0, less_than_one=0.2)
                counts += [0] * (nsym - len(counts))
                if counts[nsym - 1] == 0:                          # the last described symbol takes a cell from the richest
                    top = max(range(len(counts)), key=lambda s: counts[s])
                    assert counts[top] >= 2
                    counts[top] -= 1
                    counts[nsym - 1] = rnd.choice((1, -1))
                counts = counts[:nsym]
                lits = bytes(rnd.choice(symbols) for _ in range(rnd.randint(1, 300)))
                four = rnd.random() < 0.5 and len(lits) >= 8
                desc = tree.fse(rnd, log, counts=counts)
                body = desc + tree.streams(lits, four)
                section = lit_header(2, huf_lhl(rnd, four, len(lits), len(body)), len(lits), len(body)) + body
                f.out += lits
                f._add(2, section + b"\x00", False)
                # libzstd's workspace of 89 words (zs_huf_read): above 12 symbols at log 6, above 92 at log 5
                refuse = 1 + (1 << log) + (2 * nsym + (1 << log) + 8 + 3) // 4 > 89
                _finish(out, "nc_w_log%d_%dsym_%d" % (log, nsym, rep), fam, f, feats=() if refuse else ("w:log%d" % log, "w:%dsymbols" % nsym), refuse=refuse)
    # the weights' table at log 7: refused
    rnd, f = _start(1000 + k, prefix=0)
    tree = Tree.of(rnd, 4, list(range(40, 52)))
    counts = norm_counts(rnd, 7, sorted(set(tree.weights[:-1])), 11, spare=0)
    lits = bytes(rnd.choice(range(40, 52)) for _ in range(50))
    body = tree.fse(rnd, 7, counts=counts) + tree.streams(lits, False)
    f._add(2, lit_header(2, 0, len(lits), len(body)) + body + b"\x00", False)
    _finish(out, "nc_w_log7", fam, f, refuse=True)


def family_fse_build(out):
    fam = "fse_build"
    k = 0
    for name, idx in (("ll", 0), ("of", 1), ("ml", 2)):
        for rep in range(14):
            # many "less than one" symbols at log 5: the spread's skip rule fires again and again
            rnd, f = _start(2000 + k)
            k += 1
            nlow = rnd.randint(12, 27 if name != "of" else 24)
            low = sorted(rnd.sample(range(29), nlow))
            rich = rnd.choice([s for s in range(29) if s not in low])
            counts = [0] * 29
            for s in low:
                counts[s] = -1
            counts[rich] = 32 - nlow
            while counts[-1] == 0:
                counts.pop()
            pool = [s for s in low + [rich] if s < (18 if name == "ll" else 9 if name == "of" else 40)] or [rich]
            if name == "of" and rich >= 9 and not [s for s in low if s < 9]:
                continue
            seqs, nlit = _sym_seqs(rnd, f, name, pool, rnd.randint(2, 60))
            modes = ["predefined"] * 3
            modes[idx] = ("fse", 5, counts)
            f.compressed(simple_lits(rnd, nlit), seqs, tuple(modes), spoil=SPOIL[k & 1] if rep >= 10 else None)
            _finish(out, "build_%s_skip_%d" % (name, rep), fam, f)
        for rep in range(10):
            # a symbol whose cells have different bits each: counts of 3, 5, 6, 7 (no power of two)
            rnd, f = _start(2000 + k)
            k += 1
            log = rnd.randint(5, MAX_LOG[name])
            a, b, c = rnd.sample(range(8), 3)
            counts = [0] * 8
            counts[a] = rnd.choice((3, 5, 6, 7))
            counts[b] = rnd.choice((3, 5, 7))
            counts[c] = (1 << log) - counts[a] - counts[b]
            while counts[-1] == 0:
                counts.pop()
            seqs, nlit = _sym_seqs(rnd, f, name, [a, b, c], rnd.randint(20, 90))
            modes = [rnd.choice(("predefined", "rle")) for _ in range(3)]
            modes[idx] = ("fse", log, counts)
            for j, nm in enumerate(("ll", "of", "ml")):
                if modes[j] == "rle":                                  # one code for all: 3 literals, 5 bytes, the first repeat offset
                    seqs = [((3 if nm == "ll" else s[0]), (5 if nm == "ml" else s[1]), (0 if nm == "of" else s[2]), (0 if nm == "of" else s[3])) for s in seqs]
            nlit = sum(s[0] for s in seqs)
            f.compressed(simple_lits(rnd, nlit + 1), seqs, tuple(modes), spoil="bit_long" if rep >= 8 else None)
            _finish(out, "build_%s_uneven_bits_%d" % (name, rep), fam, f)


def _mode_seqs(rnd, f, modes, nseq, fixed):
    """sequences that fit modes: an RLE-mode or Repeat-of-RLE code stays on fixed[name]"""
    pools = {"ll": [0, 1, 2, 5, 17], "of": [0, 1, 3, 5], "ml": [0, 1, 4, 33]}
    for name, m in zip(("ll", "of", "ml"), modes):
        if m == "rle":
            fixed[name] = rnd.choice(pools[name])
        if m == "rle" or (m == "repeat" and name in fixed):
            pools[name] = [fixed[name]]
        elif m == "repeat" and name in f.tabs:
            pools[name] = [s for s in pools[name] if s in f.tabs[name].sym]
        elif m != "repeat":
            fixed.pop(name, None)
    return random_seqs(rnd, f, nseq, pools["ll"], pools["of"], pools["ml"])


def family_modes(out):
    fam = "modes"
    names = ("predefined", "rle", "fse", "repeat")
    k = 0

    def mode(rnd, m, name):
        return ("fse", rnd.randint(5, MAX_LOG[name])) if m == "fse" else m
    for idx, name in enumerate(("ll", "of", "ml")):
        for a in names:
            for b in names:
                for between in ("", "nseq0", "raw", "rle", "spoiled"):
                    if between and b != "repeat" and (between != "spoiled" or a == "repeat"):
                        continue
                    rnd, f = _start(3000 + k)
                    k += 1
                    fixed = {}
                    first = a
                    if a == "repeat":                                 # a Repeat needs something before it: three blocks
                        m0 = [rnd.choice(names[:3]) for _ in range(3)]
                        seqs, nlit = _mode_seqs(rnd, f, m0, rnd.randint(1, 12), fixed)
                        f.compressed(simple_lits(rnd, nlit), seqs, tuple(mode(rnd, m, n) for m, n in zip(m0, ("ll", "of", "ml"))))
                    m1 = [rnd.choice(names[:3]) for _ in range(3)]
                    m1[idx] = first
                    seqs, nlit = _mode_seqs(rnd, f, m1, rnd.randint(1, 12), fixed)
                    f.compressed(simple_lits(rnd, nlit), seqs, tuple(mode(rnd, m, n) for m, n in zip(m1, ("ll", "of", "ml"))))
                    if between == "nseq0":
                        f.compressed(simple_lits(rnd, 9), [])
                    elif between == "raw":
                        f.raw(rnd_bytes(rnd, 33))
                    elif between == "rle":
                        f.rle(0x51, 70)
                    m2 = [rnd.choice(names) for _ in range(3)]
                    m2[idx] = b
                    seqs, nlit = _mode_seqs(rnd, f, m2, rnd.randint(1, 12), fixed)
                    f.compressed(simple_lits(rnd, nlit + 2), seqs, tuple(mode(rnd, m, n) for m, n in zip(m2, ("ll", "of", "ml"))), spoil=SPOIL[k & 1] if between == "spoiled" else None)
                    _finish(out, "modes_%s_%s_%s%s" % (name, a, b, "_over_" + between if between else ""), fam, f)
    # mixed: LL FSE, OF Repeat, ML RLE behind a block of Predefined tables
    for rep in range(6):
        rnd, f = _start(3000 + k)
        k += 1
        fixed = {}
        seqs, nlit = _mode_seqs(rnd, f, ["predefined"] * 3, 5, fixed)
        f.compressed(simple_lits(rnd, nlit), seqs)
        m = ["fse", "repeat", "rle"]
        seqs, nlit = _mode_seqs(rnd, f, m, rnd.randint(1, 30), fixed)
        f.compressed(simple_lits(rnd, nlit), seqs, (("fse", 5 + rep % 5), "repeat", "rle"))
        _finish(out, "modes_mixed_%d" % rep, fam, f)
    # Repeat and Treeless in the first compressed block of a chunk's SECOND frame, and behind a skippable frame: refused
    for what in ("ll", "of", "ml", "treeless"):
        for gap in ("", "skippable"):
            rnd, f = _start(3000 + k)
            k += 1
            tree = Tree.of(rnd, 4, list(range(97, 110)))
            lits = bytes(rnd.choice(range(97, 110)) for _ in range(40))
            seqs, _ = random_seqs(rnd, f, 3, [2], [3], [4])
            seqs = [(2, s[1], s[2], s[3]) for s in seqs]
            f.compressed(("huf", lits, tree, False, "direct", None), seqs, (("fse", 5), ("fse", 5), ("fse", 6)))
            first = f.bytes()
            g = Frame(rnd)
            g.raw(rnd_bytes(rnd, 600, 7))
            g.tabs, g.tree = dict(f.tabs), f.tree                     # what a decoder that forgot to reset would still hold
            m = ["predefined"] * 3
            if what != "treeless":
                m[("ll", "of", "ml").index(what)] = "repeat"
            seqs, _ = random_seqs(rnd, g, 3, [2], [3], [4])
            g.compressed(("treeless", lits, False, None) if what == "treeless" else ("raw", lits, 1), seqs, tuple(m))
            skip = struct.pack("<II", 0x184D2A50 + rnd.randrange(16), 5) + b"skip!" if gap else b""
            stream = first + skip + g.bytes()
            out.append(Case("modes_second_frame_%s%s" % (what, "_behind_skippable" if gap else ""), fam, stream, None, set(), room=len(f.out) + len(g.out) + 300))
            # the same two blocks in ONE frame are accepted
            rnd, f = _start(3000 + k)
            k += 1
            seqs, _ = random_seqs(rnd, f, 3, [2], [3], [4])
            f.compressed(("huf", lits, tree, False, "direct", None), seqs, (("fse", 5), ("fse", 5), ("fse", 6)))
            seqs, _ = random_seqs(rnd, f, 3, [2], [3], [4])
            f.compressed(("treeless", lits, False, None) if what == "treeless" else ("raw", lits, 1), seqs, tuple(m))
            _finish(out, "modes_same_frame_%s%s" % (what, "_2" if gap else ""), fam, f)
    # an RLE-mode symbol above the alphabet
    for idx, (name, sym) in enumerate((("ll", 36), ("of", 32), ("ml", 53))):
        for delta in (0, 1, 100):
            rnd, f = _start(3000 + k)
            k += 1
            m = ["predefined"] * 3
            m[idx] = "rle"
            seqs, nlit = _mode_seqs(rnd, f, m, 4, {})
            spec = simple_lits(rnd, nlit)
            f.compressed(spec, seqs, tuple(m))
            kind, payload, size, last = f.blocks[-1]
            pos = len(f.literals(spec)[0]) + 2                         # behind the sequence count and the modes byte
            payload = payload[:pos] + bytes([sym + delta]) + payload[pos + 1:]
            f.blocks[-1] = (kind, payload, size, last)
            _finish(out, "modes_rle_symbol_%s_%d" % (name, sym + delta), fam, f, refuse=True)


def family_offsets(out):
    fam = "offsets"
    k = 0
    # offset codes 0, 1, 2 with each extra-bit value and literal length 0 and above: behind a prefix, then all rotations
    for code, extra in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)):
        for ll in (0, 3):
            for prior in ((), ((1, 4, 4, 9),), ((1, 4, 4, 9), (2, 5, 5, 3)), ((1, 4, 4, 9), (2, 5, 5, 3), (1, 3, 3, 2))):
                rnd, f = _start(4000 + k, prefix=200)
                k += 1
                seqs = list(prior) + [(ll, 7, code, extra), (2, 4, 0, 0), (0, 5, 1, 1), (1, 3, 1, 0)]
                f.compressed(simple_lits(rnd, sum(s[0] for s in seqs) + 1), seqs, rnd.choice((("predefined",) * 3, (("fse", 5), ("fse", 5), ("fse", 5)))))
                _finish(out, "off_code%d_%d_ll%d_after%d" % (code, extra, ll, len(prior)), fam, f)
                if len(prior) == 3 or (len(prior) == 1 and ll):        # the same with a prefix that the last rotation's offset outruns
                    rnd, f = _start(4000 + k, prefix=0)
                    k += 1
                    f.compressed(simple_lits(rnd, sum(s[0] for s in seqs) + 1), seqs, ("predefined",) * 3)
                    assert f.bad
                    _finish(out, "off_code%d_%d_ll%d_after%d_no_prefix" % (code, extra, ll, len(prior)), fam, f)
    # r1 - 1 when r1 is 1: libzstd forces 1
    for rep in range(4):
        rnd, f = _start(4000 + k, prefix=rep * 3)
        k += 1
        pre = [] if rep < 2 else [(1, 3, 2, 0)]                          # offset 1 as a real offset
        seqs = pre + [(0, 5, 1, 1), (0, 4, 1, 1)]
        if rep == 0:
            f.raw(b"q")
        f.compressed(simple_lits(rnd, 1 + 2), [(1, 3, 0, 0)] + seqs if rep < 2 else seqs, ("predefined",) * 3)
        _finish(out, "off_r1_minus_1_is_0_%d" % rep, fam, f)
    # repeat offsets 1 / 4 / 8 before any real offset, against a prefix long enough and one byte short
    for slot, need in ((0, 1), (1, 4), (2, 8)):
        for have in (need, need - 1):
            for as_block in (False, True):
                rnd, f = _start(4000 + k, prefix=0)
                k += 1
                if as_block and have:
                    f.raw(rnd_bytes(rnd, have))
                ll = 0 if as_block else have
                if slot == 0:
                    seq = (ll, 5, 0, 0) if ll else None
                elif slot == 1:
                    seq = (ll, 5, 1, 0) if ll else (0, 5, 0, 0)
                else:
                    seq = (ll, 5, 1, 1) if ll else (0, 5, 1, 0)
                if seq is None:
                    continue
                f.compressed(simple_lits(rnd, ll + 1), [seq], ("rle",) * 3 if k & 1 else ("predefined",) * 3)
                _finish(out, "off_initial_rep%d_have%d_%s" % (slot + 1, have, "block" if as_block else "literals"), fam, f)
    # repeat offsets carried over a block of 0 sequences and reset by a new frame
    for rep in range(6):
        rnd, f = _start(4000 + k, prefix=100)
        k += 1
        f.compressed(simple_lits(rnd, 6), [(2, 4, 6, 11), (2, 4, 5, 2), (2, 4, 4, 1)])
        f.compressed(simple_lits(rnd, 5), [])
        if rep & 1:
            f.rle(7, 40)
        f.compressed(simple_lits(rnd, 7), [(1, 4, 1, 1), (1, 4, 1, 0), (0, 4, 1, 0), (1, 4, 0, 0)], (("fse", 5), ("fse", 6), "rle") if rep & 2 else ("predefined",) * 3)
        _finish(out, "off_carried_%d" % rep, fam, f)
        first, data = f.bytes(), bytes(f.out)
        g = Frame(rnd)
        g.raw(rnd_bytes(rnd, 3 + rep))                                  # 3..8 bytes: the carried offsets would fit, 4 and 8 may not
        g.compressed(simple_lits(rnd, 3), [(1, 4, 1, 0), (1, 3, 1, 1)])
        out.append(Case("off_reset_by_frame_%d" % rep, fam, first + g.bytes(), None if g.bad else data + bytes(g.out), set() if g.bad else g.feat, room=len(data) + 300))
    # an offset equal to the frame's output so far, that plus 1, and one that reaches into the chunk's previous frame
    for total in (1, 2, 5, 13, 61, 125, 509, 510, 1000):
        for delta in (0, 1):
            for second in (False, True):
                rnd, f = _start(4000 + k, prefix=0)
                k += 1
                before = b""
                if second:
                    p = Frame(rnd)
                    p.raw(rnd_bytes(rnd, 700))
                    before, f0 = p.bytes(), bytes(p.out)
                f.raw(rnd_bytes(rnd, total - 1)) if total > 1 else None
                off = total + delta
                code = (off + 3).bit_length() - 1
                f.compressed(simple_lits(rnd, 2), [(1, 9, code, off + 3 - (1 << code))], ("predefined",) * 3 if k & 1 else (("fse", 6), ("fse", 7), ("fse", 8)))
                assert f.bad == bool(delta)
                out.append(Case("off_%d_of_%d%s" % (off, total, "_second_frame" if second else ""), fam, before + f.bytes(),
                                None if f.bad else (f0 if second else b"") + bytes(f.out), set() if f.bad else f.feat, room=len(f.out) + 1000))


def family_big_codes(out):
    fam = "big_codes"
    k = 0
    for of_code, ll_code, ml_code in ((15, 35, 52), (16, 35, 52), (17, 35, 52), (14, 35, 52), (0, 35, 51), (0, 34, 52), (0, 35, 50), (0, 33, 52), (1, 35, 51), (1, 35, 52), (2, 35, 51),
                                      (16, 34, 51), (17, 33, 51), (17, 34, 51), (17, 34, 52)):
        for fse in (False, True, None):
            if fse is None and of_code not in (0, 16, 17):
                continue
            rnd, f = _start(5000 + k, prefix=0)
            k += 1
            ll_bits, ml_bits = LL_BITS[ll_code], ML_BITS[ml_code]
            ll = LL_BASE[ll_code] + rnd.choice((0, (1 << ll_bits) - 20, rnd.randrange((1 << ll_bits) - 20)))      # (the block's literals: 131072 at most)
            ml = ML_BASE[ml_code] + rnd.choice((0, (1 << ml_bits) - 1, rnd.randrange(1 << ml_bits)))
            f.rle(0x33, 70000)
            f.raw(rnd_bytes(rnd, 90))
            f.rle(0x44, 66000)
            if of_code >= 2:
                lo = (1 << of_code) - 3
                hi = min((1 << of_code) - 1, len(f.out) + 2 + ll - lo)      # (2: the literals of the sequence before)
                extra = rnd.choice((0, hi, rnd.randrange(hi + 1)))
            else:
                extra = rnd.randrange(of_code + 1)
            tail = [(3, 6, 5, 7), (0, 4, 1, 1), (2, 30, 0, 0)]
            seqs = [(2, 5, 3, 1), (ll, ml, of_code, extra)] + tail
            modes = (("fse", rnd.choice((5, 6, 9))), ("fse", rnd.choice((5, 8))), ("fse", rnd.choice((5, 7, 9)))) if fse else ("predefined",) * 3
            f.compressed(("rle", 0x5A, sum(s[0] for s in seqs) + 4, 3), seqs, modes, spoil="bit_long" if fse is None else None)
            _finish(out, "big_of%d_ll%d_ml%d_%s" % (of_code, ll_code, ml_code, "spoiled" if fse is None else "fse" if fse else "predefined"), fam, f)
    # a literal length one beyond the literals; an offset one beyond the output, with the big codes
    for what in ("literals", "offset"):
        rnd, f = _start(5000 + k, prefix=0)
        k += 1
        f.rle(0x33, 66000)
        nlit = 65536 + 100
        seq = (nlit + 1, 70000, 5, 0) if what == "literals" else (nlit, 70000, 17, 66000 + nlit + 1 - ((1 << 17) - 3))
        f.compressed(("rle", 0x5A, nlit, 3), [seq], ("rle",) * 3)
        _finish(out, "big_one_beyond_%s" % what, fam, f)
        assert f.bad


def family_huffman(out):
    fam = "huffman"
    k = 0

    def one(name, rnd, f, tree, lits, four, how, lhl=None, seqs=None, refuse=False, feats=()):
        f.compressed(("huf", lits, tree, four, how, lhl), seqs or [])
        _finish(out, name, fam, f, refuse=refuse, feats=feats)
    # every table log with direct and FSE-compressed weights, one and four streams, every header format
    for hlog in range(1, 13):
        for rep in range(10):
            rnd, f = _start(6000 + k, prefix=0)
            k += 1
            nsym = rnd.randint(hlog + 1, min(1 << hlog, 120 if hlog < 8 else 250))
            direct = rep & 1 == 0

            def make(symbols):
                if hlog < 12:
                    return Tree.of(rnd, hlog, symbols)
                ws = tree_weights(rnd, hlog, len(symbols))             # weight 12 is the implied one: the largest symbol has the shortest code
                ws.remove(12)
                rnd.shuffle(ws)
                weights = [0] * (max(symbols) + 1)
                for s, w in zip(sorted(symbols), ws + [12]):
                    weights[s] = w
                return Tree(weights)
            if direct:
                symbols = rnd.sample(range(129), min(nsym, 129))
                tree, how = make(symbols), "direct"
            else:
                symbols, tree, how = fse_tree(rnd, nsym, make)
            four = rep & 2 != 0
            n = rnd.choice((1, 2, 3, 63, 64, 65, 255, 256, 257, 1023)) if not four else rnd.choice((4, 7, 8, 13, 255, 256, 257, 1023, 1024, 1025, 3000))
            lits = bytes(rnd.choice(symbols) for _ in range(n))
            while not four and len(tree.stream(lits)) + 130 >= 1024:    # (one stream: a section below 1 KiB)
                lits = lits[:len(lits) // 2]
            n = len(lits)
            lhl = None
            if four and rep & 4:
                lhl = 3 if rep == 7 else 2
            if rep >= 8:                                                # the literals are read, then the sequences are a bit long
                f.compressed(("huf", lits, tree, four, how, lhl), [(n // 2, 3, 0, 0)], spoil="bit_long")
                _finish(out, "huf_log%d_%s_%s_%d_spoiled" % (hlog, "direct" if direct else "fse", "4x" if four else "1x", n), fam, f)
                continue
            one("huf_log%d_%s_%s_%d_%d" % (hlog, "direct" if direct else "fse", "4x" if four else "1x", n, rep), rnd, f, tree, lits, four, how, lhl)
    # 2 symbols, 256 symbols (every weight equal; one symbol 255 with FSE weights), 128 direct weights
    rnd, f = _start(6000 + k, prefix=0)
    one("huf_2_symbols", rnd, f, Tree([1, 1]), bytes(rnd.randrange(2) for _ in range(77)), False, "direct")
    rnd, f = _start(6001 + k, prefix=0)
    one("huf_2_symbols_far_apart", rnd, f, Tree([0] * 5 + [1] + [0] * 122 + [1]), bytes(rnd.choice((5, 128)) for _ in range(40)), True, "direct")
    rnd, f = _start(6002 + k, prefix=0)
    one("huf_64_equal_weights", rnd, f, Tree([1] * 64), rnd_bytes(rnd, 700, 64), True, "direct")
    rnd, f = _start(6003 + k, prefix=0)
    one("huf_128_equal_weights_direct_127", rnd, f, Tree([1] * 128), rnd_bytes(rnd, 300, 128), False, "direct")
    rnd, f = _start(6004 + k, prefix=0)
    ws = tree_weights(rnd, 9, 129)
    rnd.shuffle(ws)
    one("huf_129_symbols_direct_128", rnd, f, Tree(ws), rnd_bytes(rnd, 500, 129), True, "direct")
    rnd, f = _start(6005 + k, prefix=0)
    ws = [1] * 4 + [2] * 250 + [3] * 2                              # 255 weights in under 128 bytes: nearly all alike
    rnd.shuffle(ws)
    tree = Tree(ws)
    lits = rnd_bytes(rnd, 900)
    body = tree.fse(rnd, 6, counts=[0, 4, 56, 4]) + tree.streams(lits, True)
    f._add(2, lit_header(2, 2, len(lits), len(body)) + body + b"\x00", False)
    f.out += lits
    _finish(out, "huf_256_symbols_fse", fam, f, feats=("huf:256symbols", "huf:sym255", "weights:fse", "w:log6", "huf:log9", "lh:huf2", "lit:huf4"))
    rnd, f = _start(6006 + k, prefix=0)
    one("huf_one_symbol_per_weight", rnd, f, Tree([1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]), bytes(rnd.choice((0, 1, 2, 5, 11, 11, 11, 10)) for _ in range(200)), False, ("fse", 6))
    k += 10
    # the implied last weight at each value
    for lastw in range(1, 12):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        hlog = rnd.randint(max(lastw, 2), 11)
        ws = tree_weights(rnd, hlog, hlog + 1 + rnd.randrange(min(1 << (hlog - 1), 200)) // 2, keep=lastw)
        ws.remove(lastw)
        rnd.shuffle(ws)
        tree = Tree(ws + [lastw])
        one("huf_implied_weight_%d" % lastw, rnd, f, tree, bytes(rnd.randrange(len(ws) + 1) for _ in range(90)), lastw & 1 == 0, "direct")
    # refusals of the tree description: a weight of 12, a total that makes log 13, an odd count of weight 1, none of weight 1
    for name, weights in (("weight_12", [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12]), ("log_13", [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 11, 11]),
                          ("weight_1_odd", [1, 2, 2, 3]), ("weight_1_once", [1, 3, 3]), ("no_weight_1", [2, 2, 3]), ("weight_13", [1, 1, 2, 13, 3]), ("weight_15", [15, 1, 1]), ("all_weights_0", [0, 0, 0, 1]), ("not_a_power_of_two", [1, 1, 3, 1, 1, 1, 9])):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        ex = weights[:-1]
        ex2 = ex + [0] * (len(ex) & 1)
        desc = bytes([127 + len(ex)]) + bytes((ex2[j] << 4) | ex2[j + 1] for j in range(0, len(ex2), 2))
        body = desc + b"\x35\x01"
        f._add(2, lit_header(2, 0, 3, len(body)) + body + b"\x00", False)
        _finish(out, "huf_tree_%s" % name, fam, f, refuse=True)
    # one stream with 0 literals; four streams with 5, 6 and 9 literals (the fourth segment empty or negative); a jump table whose
    # lengths exceed the section; the fourth stream 0 bytes; streams one bit short and one bit long
    tree = Tree([3, 2, 1, 1])
    for n in (0,):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        body = tree.direct() + b"\x01"
        f._add(2, lit_header(2, 0, 0, len(body)) + body + b"\x00", False)
        _finish(out, "huf_1x_0_literals", fam, f)                          # libzstd reads the tree and takes the empty stream
    for n in (5, 6, 9):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        lits = bytes(rnd.randrange(4) for _ in range(n))
        seg = (n + 3) // 4
        parts = [tree.stream(lits[j * seg:(j + 1) * seg]) for j in range(4)]
        body = tree.direct() + struct.pack("<3H", *(len(p) for p in parts[:3])) + b"".join(parts)
        f._add(2, lit_header(2, 1, n, len(body)) + body + b"\x00", False)
        f.out += lits
        _finish(out, "huf_4x_%d_literals" % n, fam, f, refuse=n == 5)        # a fourth segment of 0 literals is read; of -1 refused
    for how in ("jump_beyond", "fourth_empty", "bit_short", "bit_long", "first_empty"):
        for four in (True, False):
            if not four and how not in ("bit_short", "bit_long"):
                continue
            rnd, f = _start(6000 + k, prefix=0)
            k += 1
            lits = bytes(rnd.choice((0, 0, 0, 1, 1, 2, 3)) for _ in range(41))
            seg = 11
            parts = [tree.stream(lits[j * seg:(j + 1) * seg]) for j in range(4)] if four else [tree.stream(lits)]
            j = rnd.randrange(len(parts))
            if how == "bit_short":                                        # the last symbol's last bit is missing: drop the bit under the marker
                v = int.from_bytes(parts[j], "little") >> 1
                parts[j] = v.to_bytes(len(parts[j]), "little").rstrip(b"\x00")
            elif how == "bit_long":
                v = int.from_bytes(parts[j], "little") << 1
                parts[j] = v.to_bytes(len(parts[j]) + 1, "little").rstrip(b"\x00")
            lens = [len(p) for p in parts[:3]]
            if how == "jump_beyond":
                lens[2] += len(parts[3]) + 1
            elif how == "fourth_empty":
                lens[2] += len(parts[3])
            elif how == "first_empty":
                lens[1] += lens[0]
                lens[0] = 0
            body = tree.direct() + (struct.pack("<3H", *lens) if four else b"") + b"".join(parts)
            f._add(2, lit_header(2, 1 if four else 0, len(lits), len(body)) + body + b"\x00", False)
            _finish(out, "huf_%s_%s" % (how, "4x" if four else "1x"), fam, f, refuse=True)
    # the grid for libzstd's two stream decoders: literal counts by mean code length, four streams (the flips of these are the check)
    for n in (256, 1024, 4096, 20000, 131072):
        for mean in (1, 2, 4, 6, 8):
            if n == 131072 and mean == 8:                               # (as many bytes as literals: no block holds them)
                continue
            rnd, f = _start(6000 + k, prefix=0)
            k += 1
            # codes of several lengths at every mean, so that a flipped bit shifts what follows it; symbols drawn by 2 ** -length
            if mean == 1:
                weights, p = [6, 5, 4, 3, 2, 1, 1], [200, 20, 8, 4, 2, 1, 1]
            elif mean == 8:
                weights = [1] * 4 + [2] * 250 + [3] * 2
            else:
                weights = {2: [4, 3, 2, 1, 1], 4: [5] * 2 + [3] * 4 + [2] * 4 + [1] * 8, 6: [4] * 16 + [2] * 32 + [1] * 64}[mean]
            if mean > 1:
                p = [1 << w for w in weights]
            tree = Tree(weights)
            lits = bytes(rnd.choices(range(len(weights)), p, k=n))
            f.compressed(("huf", lits, tree, True, "direct" if len(weights) <= 129 else ("fse", 6, [0, 4, 56, 4]), None), [])
            _finish(out, "huf_grid_%d_by_%d" % (n, mean), fam, f, checksum=False)
    # Treeless: behind one and four streams, with another stream count, every header format, across raw / RLE blocks and a block with
    # raw literals; behind a block whose Huffman section was refused nothing follows (the frame has ended), so: behind a FRAME that
    # was refused is another chunk; and Treeless behind a block with only raw literals in a fresh frame: refused
    for rep in range(24):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        hlog = rnd.randint(1, 11)
        symbols, tree, how = fse_tree(rnd, rnd.randint(hlog + 1, min(1 << hlog, 100)), lambda symbols: Tree.of(rnd, hlog, symbols))
        if max(symbols) <= 128 and rep & 1:
            how = "direct"
        four = rep & 1 == 0
        f.compressed(("huf", bytes(rnd.choice(symbols) for _ in range(rnd.randint(8, 300))), tree, four, how, None), [])
        if rep & 2:
            f.raw(b"between")
        if rep & 4:
            f.compressed(simple_lits(rnd, 12), [(3, 4, 2, 0)])
        if rep & 8:
            f.rle(9, 9)
        n = rnd.choice((1, 7, 64, 300, 1023)) if rep % 3 else rnd.choice((8, 13, 257, 1021))
        four2 = rep % 3 == 0
        lhl = None if not four2 else (3, 2, 1)[rep // 3 % 3]
        seqs = [(1, 3, 0, 0), (0, 4, 1, 0)] if rep & 1 else []
        f.compressed(("treeless", bytes(rnd.choice(symbols) for _ in range(n)), four2, lhl), seqs)
        _finish(out, "huf_treeless_%d" % rep, fam, f)
    for rep in range(3):
        rnd, f = _start(6000 + k, prefix=0)
        k += 1
        f.compressed(simple_lits(rnd, 20), [(3, 4, 2, 0)])
        if rep:
            f.compressed(("rle", 65, 40, 1), [])
        f.compressed(("treeless", b"abc", rep == 2, None), [])
        _finish(out, "huf_treeless_without_tree_%d" % rep, fam, f)
        assert f.bad


def family_frames(out):
    fam = "frames"
    k = 0

    def header(fcs_len, value, single=False, wd=0x58, reserved=False):
        code = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_len]
        assert fcs_len != 1 or single
        fhd = (code << 6) | (0x20 if single else 0) | (8 if reserved else 0)
        return bytes([fhd]) + (b"" if single else bytes([wd])) + (value.to_bytes(fcs_len, "little") if fcs_len else b"")
    # Frame_Content_Size in its four forms, exact, one too large, one too small; the 8-byte form with a non-zero high word
    for fcs_len, n in ((1, 0), (1, 200), (1, 255), (2, 256), (2, 300), (2, 65791), (4, 70000), (4, 5), (8, 90), (8, 66000)):
        for delta in (0, 1, -1, 1 << 32):
            if delta == (1 << 32) and fcs_len != 8 or n + delta < 0:
                continue
            for single in ((True,) if fcs_len == 1 else (False, True)):
                rnd, f = _start(7000 + k, prefix=0)
                k += 1
                if n > 1000:
                    f.rle(0x11, n - 300)
                    f.raw(rnd_bytes(rnd, 200))
                    f.compressed(simple_lits(rnd, 40), [(5, 60, 4, 2)])
                elif n > 20:
                    f.raw(rnd_bytes(rnd, n - 20))
                    f.compressed(simple_lits(rnd, 10), [(5, 10, 3, 2)])
                elif n:
                    f.raw(rnd_bytes(rnd, n))
                else:
                    f.raw(b"")
                assert len(f.out) == n
                v = n + delta - (256 if fcs_len == 2 else 0)
                if not 0 <= v < (1 << (8 * fcs_len)):
                    continue
                _finish(out, "frame_fcs%d_%d%+d%s" % (fcs_len, n, delta, "_single" if single else ""), fam, f, header=header(fcs_len, v, single), refuse=delta != 0,
                        feats=() if delta else ("fcs:%d" % fcs_len, "frame:single" if single else "frame:window"))
    # window descriptors, the reserved bit
    for wd, ok in ((0x00, True), (0xA8, True), (0xAF, True), (0xB0, False), (0xF8, False)):
        for fcs_len in (0, 4):
            rnd, f = _start(7000 + k, prefix=50)
            k += 1
            f.compressed(simple_lits(rnd, 10), [(5, 10, 3, 2)])
            _finish(out, "frame_window_0x%02x_fcs%d" % (wd, fcs_len), fam, f, header=header(fcs_len, len(f.out), wd=wd), refuse=not ok, feats=("wd:0x%02x" % wd,) if ok else ())
    # libzstd's two sequence decoders: windows of 16 MiB (its usual one) and above (the prefetching one, for more than 4 sequences
    # and an offset table with 7 / 256 of its cells above 22 bits): bits left over, accepted by the second alone; an over-read four
    # sequences ahead, refused by it; an error in a sequence that it has not reached yet
    far = [6, 6, 6, 5, 4, 2, 2] + [0] * 16                                  # offset codes 0..6 and 23: the cells of code 23 by log
    for wd in (0x70, 0x71, 0x78, 0xA8):
        for nseq in (4, 5, 9):
            for of_mode in ("predefined", ("fse", 5, far + [1]), ("fse", 8, [c * 8 for c in far[:6]] + [18] + [0] * 16 + [6]), ("fse", 8, [c * 8 for c in far[:6]] + [17] + [0] * 16 + [7]), ("fse", 6)):
                for spoil in (None, "bit_long", "cut_tail", "late_error"):
                    rnd = random.Random(7000 + k)
                    k += 1
                    f = Frame(rnd, long_window=wd > 0x70)
                    f.raw(rnd_bytes(rnd, 200, 9))
                    seqs, nlit = random_seqs(rnd, f, nseq, [0, 1, 2, 16], [0, 1, 2, 3, 4, 5], [0, 3, 32])
                    if spoil == "late_error":                           # the last sequence's offset is beyond the output
                        last = seqs[-1]
                        seqs[-1] = (last[0], last[1], 6, 63)
                    if spoil == "cut_tail":
                        t = Table(*DEFAULT["of"]) if of_mode == "predefined" else Table(of_mode[1], of_mode[2]) if len(of_mode) > 2 else None
                        if not (f.long_window and nseq > 4 and t is not None and (sum(1 for x in t.sym if x > 22) << (8 - t.log)) >= 7):
                            continue
                    f.compressed(simple_lits(rnd, nlit + 3), seqs, ("predefined", of_mode, rnd.choice(("predefined", ("fse", 6)))), spoil=spoil if spoil != "late_error" else None)
                    mname = of_mode if isinstance(of_mode, str) else "fse%d_%d" % (of_mode[1], of_mode[2][-1] if len(of_mode) > 2 else 0)
                    _finish(out, "frame_decoders_0x%02x_%dseq_%s_%s" % (wd, nseq, mname, spoil or "plain"), fam, f, header=header(0, 0, wd=wd))
    for single in (False, True):
        rnd, f = _start(7000 + k, prefix=50)
        k += 1
        _finish(out, "frame_reserved_bit%s" % ("_single" if single else ""), fam, f, header=header(1 if single else 0, 50, single, reserved=True), refuse=True)
    # a chunk of 8 frames with skippable frames of length 0 between them; with one frame of them broken
    for broken in (None, 0, 3, 7):
        rnd = random.Random(7000 + k)
        k += 1
        stream, data, feat, bad = b"", b"", set(), False
        for j in range(8):
            f = Frame(rnd)
            f.raw(rnd_bytes(rnd, 20 + j))
            seqs, nlit = random_seqs(rnd, f, 4, [0, 1, 3], [0, 1, 2, 3], [2] if j & 1 else [0, 2, 7])
            f.compressed(simple_lits(rnd, nlit), seqs, (("fse", 5), "predefined", "rle") if j & 1 else ("predefined",) * 3) if j != 5 else f.rle(j, 100)
            if j == broken:
                f.compressed(("raw", b"ab", 0), [(3, 3, 0, 0)], ("rle",) * 3)
                bad = True
            stream += f.bytes(checksum=bool(j & 1)) + struct.pack("<II", 0x184D2A50 + j, 0)
            data += bytes(f.out)
            feat |= f.feat
        out.append(Case("frame_8_frames%s" % ("" if broken is None else "_broken_%d" % broken), fam, stream, None if bad else data, set() if bad else feat | {"chunk:8frames", "chunk:skippable0"}, room=len(data) + 300))
    # a compressed block of 131071 bytes, and one of 131072; RLE literals of 131072 and 131073
    for size in (131071, 131072):
        rnd, f = _start(7000 + k, prefix=0)
        k += 1
        seqs = [(4, 5, 2, 0), (1, 3, 0, 0)]
        tail_len = len(Frame(random.Random(1)).compressed(("raw", b"", 0), seqs)) - 1
        nlit = size - tail_len - 3
        f.compressed(("raw", rnd_bytes(random.Random(k), 1000) * (nlit // 1000) + bytes(nlit % 1000), 3), seqs)
        assert f.blocks[-1][2] == size, f.blocks[-1][2]
        _finish(out, "frame_block_of_%d" % size, fam, f, refuse=size == 131072)
    for n in (131072, 131073):
        for lhl in (3,):
            rnd, f = _start(7000 + k, prefix=0)
            k += 1
            f.compressed(("rle", 0x77, n, 3), [(n - 10, 3, 2, 0)], ("rle",) * 3)
            _finish(out, "frame_rle_literals_%d" % n, fam, f, refuse=n > 131072)
    # RLE and raw literal headers in their three formats
    for kind in ("raw", "rle"):
        for lhl, n in ((0, 1), (0, 30), (2, 17), (1, 0), (1, 31), (1, 4095), (3, 0), (3, 4096), (3, 20)):
            rnd, f = _start(7000 + k, prefix=0)
            k += 1
            spec = ("raw", rnd_bytes(rnd, n), lhl) if kind == "raw" else ("rle", 0x30 + lhl, n, lhl)
            f.compressed(spec, [(n // 2, 3, 0, 0)] if n > 1 else [])
            _finish(out, "frame_%s_literals_format%d_%d" % (kind, lhl, n), fam, f)
    # an empty last block of each type
    for kind in ("raw", "rle", "compressed", "compressed_short"):
        for first in (False, True):
            rnd, f = _start(7000 + k, prefix=0 if first else 40)
            k += 1
            if kind == "raw":
                f.raw(b"")
            elif kind == "rle":
                f.rle(1, 0)
            elif kind == "compressed":
                f._add(2, b"", False)                                   # a compressed block of 0 bytes: refused (below 3)
            else:
                f._add(2, b"\x00\x00", False)                           # ... of 2 bytes: no literals, no sequences; still below 3
            _finish(out, "frame_empty_last_%s%s" % (kind, "_only" if first else ""), fam, f, refuse=kind.startswith("compressed"), feats=() if kind.startswith("compressed") else ("block:empty_" + kind,))


_all = None


def cases():
    global _all
    if _all is None:
        out = []
        for fn in (family_ncount, family_fse_build, family_modes, family_offsets, family_big_codes, family_huffman, family_frames):
            fn(out)
        names = [c.name for c in out]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
        assert {"huf_implied_weight_%d" % w for w in range(1, 12)} <= set(names)
        assert sum(n.startswith("huf_log") for n in names) == 120 and sum(n.startswith("huf_treeless_") for n in names) == 24 + 3
        _all = out
    return _all


def flips(n, seed=17):
    """n seeded single-bit flips, spread over the families and their cases: [(name, family, stream, the case flipped)]"""
    rnd = random.Random(seed)
    by = {}
    for c in cases():
        by.setdefault(c.family, []).append(c)
    out = []
    fams = sorted(by)
    for i in range(n):
        c = rnd.choice(by[fams[i % len(fams)]])
        at = rnd.randrange(8 * len(c.stream))
        b = bytearray(c.stream)
        b[at >> 3] ^= 1 << (at & 7)
        out.append(("flip_%d_%s_bit%d" % (i, c.name, at), c.family, bytes(b), c))
    return out


def grid_flips():
    """every point of the Huffman grid (huf_grid_*) with a fixed set of 20 single-bit flips where libzstd's two stream decoders end
    differently: per stream three of its first 32 bits (the symbols decoded LAST), one bit of its last byte (the marker), and four
    bits of the jump table: [(name, family, stream, the case flipped)]"""
    out = []
    for c in cases():
        if not c.name.startswith("huf_grid_"):
            continue
        s, at = c.stream, 9                                               # magic, descriptor, window, block header
        lhl = (s[at] >> 2) & 3
        lh, nb = (3, 3, 4, 5)[lhl], (10, 10, 14, 18)[lhl]
        lcs = (int.from_bytes(s[at:at + lh], "little") >> (4 + nb)) & ((1 << nb) - 1)
        jump = at + lh + (1 + s[at + lh] if s[at + lh] < 128 else 1 + (s[at + lh] - 126) // 2)
        lens = list(struct.unpack_from("<3H", s, jump))
        lens.append(at + lh + lcs - jump - 6 - sum(lens))
        assert min(lens) >= 4 and s[jump + 6 + sum(lens)] == 0           # (the sequence count behind the literals)
        rnd = random.Random(c.name)
        where, start = [(jump + rnd.randrange(6), rnd.randrange(8)) for _ in range(4)], jump + 6
        for n in lens:
            where += [(start + b // 8, b % 8) for b in rnd.sample(range(32), 3)] + [(start + n - 1, rnd.randrange(8))]
            start += n
        for byte, bit in where:
            b = bytearray(s)
            b[byte] ^= 1 << bit
            out.append(("gridflip_%s_byte%d_bit%d" % (c.name, byte, bit), c.family, bytes(b), c))
    return out


def digest(b):
    """the first 128 bits of SHA-256, base64: what golden_zstd_synth.json holds of a stream and of an output"""
    return base64.urlsafe_b64encode(hashlib.sha256(bytes(b)).digest()[:16]).decode().rstrip("=")


def recorded_entries():
    """what tests/golden/golden_zstd_synth.json holds (the GPU tests do not call libzstd), per case, per flip of flips(600) and per flip of grid_flips(), in
    their order: [digest of the stream, exact capacity, libzstd's results at the four capacities, digest of the output at the exact
    capacity (absent where libzstd refuses there)]; no streams and no names"""
    out = []
    for s, cap in [(c.stream, c.cap) for c in cases()] + [(f[2], f[3].cap) for f in flips(600) + grid_flips()]:
        v = [Z.zstd_verdict(s, k) for k in Z.capacities(cap)]
        out.append([digest(s), cap, [r for r, _ in v]] + ([digest(v[0][1])] if v[0][0] >= 0 else []))
    return out
