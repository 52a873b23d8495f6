"""The input sweep's cases (tests/test_input_sweep_model.py on the CPU, tests/test_input_sweep_gpu.py on the GPU): the capacity sweep's
sibling (tests/capacity_cases.py, whose bodies, block writers and `render` it uses) on the input side.  Three families, one chunk per case:

  A  where the input ends: in_len cut at every value of [0, 40) and [len - 40, len] and at -2 .. +23 around the token of eight chosen
     sequences, each cut twice: `after` (the bytes packed behind in_len, see pack in tests/device_batch.py) is once the stream's
     own continuation and once 0xFF bytes — a length-extension chain read past the end runs on, an offset read there is 65 535;
  B  the offset at its edges: 0, small values, the match start ms and the values around it, 65 535 (Snappy: in every copy form that holds
     the value, and above 65 535 in the 4-byte form); with a dictionary ms + 1 .. ms + its length + 1; the Snappy preamble's forms;
  C  the overlap grid: 1 457 (period, match length) pairs dealt over streams that fit each window, in eight variants that turn every
     pair through all destination alignments modulo 8; all valid.

Everything is seeded; expected (result, bytes) come from the CPU oracle (with a dictionary: tests/lz4_dict_model.py; the size query:
batch_sizes_cases.expected_size), never from a GPU path.  No GPU needed to import this."""
import functools

import numpy as np

import batch_sizes_cases as B
import capacity_cases as K
import lz4_dict_model as D
import oracle

AFTER = 48                                         # bytes of `after` behind every family-A cut
A_TAILS = ((None, 0), (None, 4), (None, 5), (None, 13), (None, 16), (None, 270), (19, 6))
EXT_TAILS = tuple((1030, k) for k in (1, 2, 3, 4))  # a last match with four length bytes: `ip + 4 > iend` decides only behind three or more
ROOMS = (0, 64)                                    # out_cap = U and U + 64
BOUNDS = (32768, 65536, 98304)                     # the slabs' boundaries of a big chunk
DICT_LEN = 4096


def _pick(streams, tails=A_TAILS):
    names = {"match%s/tail%d" % t for t in tails}
    return [s for s in streams if s["name"].split("/", 1)[1] in names]


def _case(s, blob, cap, r, o, **extra):
    return dict(K._case(s, blob, cap, r, o), **extra)


def lz4_tokens(seqs):
    """the input position of every sequence's token and of its offset field in K._lz4_block(seqs, ...)"""
    out, ip = [], 0
    for lit, _, m in seqs:
        at = ip + 1 + K._ext_bytes(len(lit), 15) + len(lit)
        out.append((ip, at))
        ip = at + 2 + K._ext_bytes(m - 4, 15)
    return out


def snappy_walk(e):
    """[(input position, output position)] of every element of an element stream, and the pair behind the last one"""
    out, ip, op = [], 0, 0
    while ip < len(e):
        out.append((ip, op))
        tag = e[ip]; kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1; nb = max(ln - 60, 0); ip += 1
            if nb: ln = int.from_bytes(e[ip:ip + nb], "little") + 1
            ip += nb + ln; op += ln
        else:
            op += ((tag >> 2) & 7) + 4 if kind == 1 else (tag >> 2) + 1
            ip += (0, 2, 3, 5)[kind]
    assert ip == len(e)
    return out + [(ip, op)]


def cut_lens(n, tokens, head=True):
    s = set(range(n - 40, n + 1)) | (set(range(40)) if head else set())
    for t in tokens:
        s |= set(range(t - 2, t + 24))
    return sorted(k for k in s if 0 <= k <= n)


def _afters(full, k):
    return (("own", full[k:k + AFTER]), ("ff", b"\xff" * AFTER))


def _crossing(pos):
    """the sequences whose output crosses one of BOUNDS"""
    return [next(j for j, (ls, _, me) in enumerate(pos) if ls <= b < me) for b in BOUNDS]


# ---- family A ---------------------------------------------------------------------------------------------------------------------------
def _a_lz4(s, full, tokens, head=True):
    out = []
    for k in cut_lens(len(full), tokens, head):
        for room in ROOMS:
            r, o = K._lz4_raw(full[:k], s["U"] + room)
            for kind, after in _afters(full, k):
                out.append(_case(s, full[:k], s["U"] + room, r, o, after=after, kind=kind, in_len=k))
    return out


@functools.lru_cache(maxsize=None)
def a_lz4_streams(body):
    """the issue's tails of bodies a and b; body a also with EXT_TAILS; "long" with 13 final literals"""
    if body == "long": return _pick(K.lz4_streams(body), ((None, 13),))
    out = _pick(K.lz4_streams(body))
    if body == "a":
        more = K._streams(K.sequences(K._SEEDS[body]), K._SEEDS[body], tails=list(EXT_TAILS))
        for s in more: s["bytes"] = K._lz4_block(s["seqs"], s["tail"])
        out = out + more
    return out


@functools.lru_cache(maxsize=None)
def a_lz4_cases(body):
    """... the cuts of "long" also around its middle sequence, the one with two-byte length extensions"""
    out = []
    for s in a_lz4_streams(body):
        tok = lz4_tokens(s["seqs"])
        out += _a_lz4(s, s["bytes"], [tok[j][0] for j in K.CUTS + ((K.NSEQ // 2,) if body == "long" else ())])
    return out


def _a_snappy(s, tokens, head=True):
    """the cuts under the true preamble, and for a cut on an element boundary the prefix under a preamble that declares what it decodes to"""
    e = s["elements"]
    hdr = K.varint(s["U"])
    full = hdr + e
    ends = dict(snappy_walk(e))
    out = []
    for k in cut_lens(len(full), [len(hdr) + t for t in tokens], head):
        for room in ROOMS:
            r, o = oracle.snappy_decompress(full[:k], s["U"] + room)
            for kind, after in _afters(full, k):
                out.append(_case(s, full[:k], s["U"] + room, r, o, after=after, kind=kind, in_len=k, declared="true"))
        p = ends.get(k - len(hdr), 0)
        if p:
            blob = K.varint(p) + e[:k - len(hdr)]
            for room in ROOMS:
                r, o = oracle.snappy_decompress(blob, p + room)
                for kind, after in _afters(full, k):
                    out.append(_case(s, blob, p + room, r, o, after=after, kind=kind, in_len=len(blob), declared="prefix", cut=k))
    return out


def _snappy_tokens(s, pos, js):
    w = snappy_walk(s["elements"])
    return [next(ip for ip, op in w if op >= pos[j][0]) for j in js]


@functools.lru_cache(maxsize=None)
def a_snappy_cases(body):
    out = []
    for s in _pick(K.snappy_streams(body)):
        out += _a_snappy(s, _snappy_tokens(s, K.render(s["seqs"], s["tail"])[1], K.CUTS))
    return out


@functools.lru_cache(maxsize=None)
def a_big_cases(codec):
    s = K.big_streams()
    pos = K.render(s["seqs"], s["tail"])[1]
    js = _crossing(pos)
    if codec == "lz4":
        tok = lz4_tokens(s["seqs"])
        return _a_lz4(s, s["bytes"], [tok[j][0] for j in js], head=False)
    return _a_snappy(s, _snappy_tokens(s, pos, js), head=False)


# ---- family B ---------------------------------------------------------------------------------------------------------------------------
def edge_offsets(ms):
    return [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, ms - 1, ms, ms + 1, ms + 2, 65535]


def _tail13(streams):
    return _pick(streams, ((None, 13),))[0]


def _b_lz4(s, js, offsets, d=b""):
    pos = K.render(s["seqs"], s["tail"], d)[1]
    out = []
    for j in js:
        ms = pos[j][1]
        for off in offsets(ms):
            sq = list(s["seqs"])
            sq[j] = (sq[j][0], off, sq[j][2])
            blob = K._lz4_block(sq, s["tail"])
            for room in ROOMS:
                r, o = D.decode(blob, s["U"] + room, d) if d else K._lz4_raw(blob, s["U"] + room)
                out.append(_case(s, blob, s["U"] + room, r, o, seq=j, off=off, ms=ms, dict_len=len(d)))
    return out


@functools.lru_cache(maxsize=None)
def b_lz4_cases(body):
    return _b_lz4(_tail13(K.lz4_streams(body)), K.CUTS, edge_offsets)


@functools.lru_cache(maxsize=None)
def b_dict_cases(body):
    """... and ms + 1 .. ms + dictionary length + 1 at their edges: the first two values, the one that starts at the dictionary's second
    byte, at its first byte, and one before it (refused)"""
    return _b_lz4(_tail13(K.lz4_streams(body, DICT_LEN)), K.CUTS,
                  lambda ms: edge_offsets(ms) + [ms + DICT_LEN - 1, ms + DICT_LEN, ms + DICT_LEN + 1], D.dictionary(DICT_LEN))


def _copy(off, m, form):
    """one sequence's match as copy elements of one form (1: 4 .. 11 bytes, an 11-bit offset; 2: a 2-byte offset; 3: a 4-byte offset)"""
    out, top = bytearray(), 11 if form == 1 else 64
    while m > 0:
        k = min(m, top)
        if 0 < m - k < 4: k = m - 4
        if form == 1: out += bytes((((off >> 8) << 5) | ((k - 4) << 2) | 1, off & 255))
        elif form == 2: out += bytes((((k - 1) << 2) | 2, off & 255, off >> 8))
        else: out += bytes((((k - 1) << 2) | 3,)) + off.to_bytes(4, "little")
        m -= k
    return bytes(out)


def _b_snappy(s, js, offsets, seed):
    pos = K.render(s["seqs"], s["tail"])[1]
    out = []
    for j in js:
        lit, _, m = s["seqs"][j]
        ms = pos[j][1]
        head = K.snappy_elements(s["seqs"][:j] + [(lit, 1, 0)], b"", seed)          # (a match of 0 bytes: the literal alone)
        rest = K.snappy_elements(s["seqs"][j + 1:], s["tail"], seed + 1)
        for off in offsets(ms):
            for form in (1, 2, 3):
                if off >= (2048, 65536, 1 << 32)[form - 1] or (form < 3 and off > 65535): continue
                blob = K.varint(s["U"]) + head + _copy(off, m, form) + rest
                for room in ROOMS:
                    r, o = oracle.snappy_decompress(blob, s["U"] + room)
                    out.append(_case(s, blob, s["U"] + room, r, o, seq=j, off=off, ms=ms, form=form, dict_len=0))
    return out


@functools.lru_cache(maxsize=None)
def b_snappy_cases(body):
    return _b_snappy(_tail13(K.snappy_streams(body)), K.CUTS, lambda ms: edge_offsets(ms) + [65536, 0x10000 + ms, 0xFFFFFFFF], K._SEEDS[body])


@functools.lru_cache(maxsize=None)
def b_big_cases(codec):
    """one sequence behind 65 536 and one behind 98 304 of the ~100 KiB stream"""
    s = K.big_streams()
    pos = K.render(s["seqs"], s["tail"])[1]
    js = [next(j for j, p in enumerate(pos) if p[1] > b + 300) for b in BOUNDS[1:]]
    if codec == "lz4":
        return _b_lz4(s, js, lambda ms: [65534, 65535])
    return _b_snappy(s, js, lambda ms: [65536, ms, ms + 1], 21)


def preambles(u):
    """(name, preamble bytes): the forms of the declared length in front of one element stream"""
    out = [("minimal", K.varint(u))]
    for n in range(2, 12):                                                         # the same value in n bytes: padded with 0x80 .. 0x00
        b = [(u >> (7 * i)) & 127 for i in range(n)]
        out.append(("%d-bytes" % n, bytes([x | 128 for x in b[:-1]] + [b[-1]])))
    out += [("2^32-1", bytes.fromhex("ffffffff0f")), ("33-bits", bytes.fromhex("ffffffff1f")), ("2^32", bytes.fromhex("8080808010")), ("lone-80", b"\x80")]
    return out


@functools.lru_cache(maxsize=None)
def b_preamble_cases():
    """each at out_cap = U + 8; `size` is what the header size query answers.  A lone 0x80 and nothing come with and without elements."""
    s = _tail13(K.snappy_streams("a"))
    blobs = [(name, p + s["elements"]) for name, p in preambles(s["U"])] + [("lone-80-alone", b"\x80"), ("nothing", b""), ("elements-alone", s["elements"])]
    return [_case(s, blob, s["U"] + 8, *oracle.snappy_decompress(blob, s["U"] + 8), form=name, size=int(oracle.snappy_decompress_len(blob)) if blob else 0)
            for name, blob in blobs]


# ---- family C ---------------------------------------------------------------------------------------------------------------------------
PERIODS = tuple(range(1, 41)) + (63, 64, 65, 66, 127, 128, 129)
MATCHES = tuple(range(4, 10)) + tuple(range(15, 21)) + (31, 32, 33, 34, 40, 63, 64, 65, 66, 127, 128, 129, 130, 255, 274, 511, 512, 513, 1030)
VARIANTS = 8
MIN_SEQS = 300
C_DICT_MATCHES = 40                                 # with a dictionary: the first forty grid matches of a stream begin inside its end


@functools.lru_cache(maxsize=None)
def grid_pairs():
    pairs = [(p, m) for p in PERIODS for m in MATCHES]
    rng = np.random.default_rng(1900)
    return [pairs[i] for i in rng.permutation(len(pairs))]


def _overlap_stream(win, k, nstreams, v, dict_len):
    """stream k of nstreams, variant v: its share of the shuffled pairs (pair i goes to stream i mod nstreams) among plain sequences, the
    literals in front of grid match i chosen so that its destination is i + v modulo 8"""
    pairs = grid_pairs()
    mine = list(range(k, len(pairs), nstreams))
    rng = np.random.default_rng(190000 + win + k)                                   # (the same for every variant: only the literal lengths differ)
    items = mine + [-1] * max(MIN_SEQS - len(mine), 0)
    items = [items[i] for i in rng.permutation(len(items))]
    seqs, grid, op, ngrid = [], [], 0, 0
    for n, i in enumerate(items):
        ll = 64 if n == 0 else 0
        if i < 0:
            ll += int(rng.integers(0, 4)); m = int(rng.integers(4, 9))
            off = int(rng.integers(16, min(op + ll, 65535) + 1))                     # far and not overlapping
        else:
            off, m = pairs[i]
            ll += (i + v - op - ll) % 8
            if op + ll < off: ll += (off - op - ll + 7) // 8 * 8
            if dict_len and ngrid < C_DICT_MATCHES:
                off = op + ll + 1 + ngrid % off                                      # 1 .. period bytes inside the dictionary's end
            grid.append((len(seqs), pairs[i][0], m, i)); ngrid += 1
        seqs.append((rng.integers(0, 256, ll, dtype=np.uint8).tobytes(), off, m))
        op += ll + m
    tail = rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
    d = D.dictionary(dict_len) if dict_len else b""
    raw, pos = K.render(seqs, tail, d)
    return dict(name="overlap%d/%s%d.%d" % (win, "dict/" if dict_len else "", k, v), seqs=seqs, tail=tail, raw=raw, pos=pos, U=len(raw), final_lits=13, grid=grid,
                variant=v, bytes=K._lz4_block(seqs, tail), elements=K.snappy_elements(seqs, tail, 1900 + k))


def _fits(s, win):
    return s["U"] + 64 <= win and max(len(s["bytes"]), len(s["elements"]) + 3) <= win - 32


@functools.lru_cache(maxsize=None)
def overlap_streams(win, dict_len=0):
    """as few streams as keeps every variant of each inside the window (with 64 bytes of room)"""
    n = sum(m for _, m in grid_pairs()) // win + 1
    while True:
        out = []
        for k in range(n):
            for v in range(VARIANTS):
                out.append(_overlap_stream(win, k, n, v, dict_len))
                if not _fits(out[-1], win): break
            else: continue
            break
        else: return out
        n += 1


def _room(s):
    return 64 * (s["variant"] & 1)                                                   # out_cap = U and U + 64, by variant


@functools.lru_cache(maxsize=None)
def c_lz4_cases(win):
    return [_case(s, s["bytes"], s["U"] + _room(s), *K._lz4_raw(s["bytes"], s["U"] + _room(s))) for s in overlap_streams(win)]


@functools.lru_cache(maxsize=None)
def c_snappy_cases(win):
    out = []
    for s in overlap_streams(win):
        blob = K.varint(s["U"]) + s["elements"]
        out.append(_case(s, blob, s["U"] + _room(s), *oracle.snappy_decompress(blob, s["U"] + _room(s))))
    return out


@functools.lru_cache(maxsize=None)
def c_dict_cases():
    d = D.dictionary(DICT_LEN)
    return [_case(s, s["bytes"], s["U"] + _room(s), *D.decode(s["bytes"], s["U"] + _room(s), d)) for s in overlap_streams(65536, DICT_LEN)]


BIG_PERIODS = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 33, 65)
BIG_MATCHES = (66, 600)
BIG_STARTS = (1, 7, 8, 33)


@functools.lru_cache(maxsize=None)
def big_overlap_streams():
    """the ~100 KiB body with, for each (period, length, start), one such match put in `start` bytes before each of BOUNDS — one match can
    begin at a given place of a stream, so one stream per triple (96), each with its three matches"""
    base = K.sequences(21, K.BIG_NSEQ)
    rng = np.random.default_rng(1921)
    out = []
    for p in BIG_PERIODS:
        for m in BIG_MATCHES:
            for st in BIG_STARTS:
                seqs = list(base)
                for b in BOUNDS:
                    ends = np.cumsum([len(l) + n for l, _, n in seqs])
                    i = int(np.searchsorted(ends, b - st, side="right"))
                    gap = b - st - (int(ends[i - 1]) if i else 0)
                    seqs.insert(i, (rng.integers(0, 256, gap, dtype=np.uint8).tobytes(), p, m))
                tail = rng.integers(0, 256, 13, dtype=np.uint8).tobytes()
                raw, pos = K.render(seqs, tail)
                out.append(dict(name="bigoverlap/p%d/m%d/-%d" % (p, m, st), seqs=seqs, tail=tail, raw=raw, pos=pos, U=len(raw), final_lits=13, start=st, period=p, match=m,
                                bytes=K._lz4_block(seqs, tail), elements=K.snappy_elements(seqs, tail, 1921)))
    return out


@functools.lru_cache(maxsize=None)
def c_big_cases(codec):
    out = []
    for n, s in enumerate(big_overlap_streams()):
        cap = s["U"] + 64 * (n & 1)
        blob = s["bytes"] if codec == "lz4" else K.varint(s["U"]) + s["elements"]
        out.append(_case(s, blob, cap, *(K._lz4_raw(blob, cap) if codec == "lz4" else oracle.snappy_decompress(blob, cap))))
    return out


# ---- the raw-LZ4 size query on the LZ4 cases of families A and B -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def size_cases():
    """one case per distinct (stream bytes, after) of the LZ4 cases of A and B, the big stream's included: result = the decoded size
    with room that never runs out (batch_sizes_cases.expected_size), cap 0: the query takes no output"""
    seen, out = {}, []
    lists = [a_lz4_cases(b) for b in K.LZ4_BODIES] + [a_big_cases("lz4")] + [b_lz4_cases(b) for b in K.LZ4_BODIES[:2]] + [b_big_cases("lz4")]
    for c in (c for cs in lists for c in cs):
        key = (c["bytes"], c.get("after", b""))
        if key in seen: continue
        if c["bytes"] not in seen: seen[c["bytes"]] = B.expected_size(c["bytes"])
        seen[key] = True
        out.append(dict(c, cap=0, result=seen[c["bytes"]], out=b""))
    return out
