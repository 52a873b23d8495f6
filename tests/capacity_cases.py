"""The capacity sweep's cases (tests/test_capacity_model.py on the CPU, tests/test_capacity_gpu.py on the GPU): hand-built LZ4 blocks and
Snappy raw streams of 300 sequences — enough for every window's workgroup decoder (256 / 128 / 64 sequences on 64 / 32 / 16 KiB) —, each
with a family of tails, each decoded at ~270 capacities: around the decoded size U, a few tiny values, and around the literal start, the
match start and the match end of eight chosen sequences.  One chunk is one (stream, capacity) pair.  For Snappy the variable is the length
the preamble declares (out_cap = that value), and in a second pass out_cap alone under the true preamble.  Everything is seeded; the
expected (result, bytes) of every case come from the CPU oracle (with a dictionary: from tests/lz4_dict_model.py), never from a GPU path.
No GPU needed to import this."""
import functools

import numpy as np

import oracle

LITS = (0, 1, 2, 3, 5, 14, 15, 16, 30)
MLENS = (4, 5, 7, 18, 19, 20, 40)
NSEQ = 300
CUTS = (1, 2, 100, 255, 256, 257, 298, 299)       # sequences (0-based) whose literal start / match start / match end get capacities around them
BIG_NSEQ = 3900                                  # ~100 KiB decoded
# (what the last match is replaced by or None, final literals): 0 .. 13 final literals; a last literal length with an extension byte
# (15, 16) and with two (270); a last MATCH with an extension byte (19) and with two (274) in front of 4, 5 and 6 final literals
TAILS = [(None, k) for k in range(14)] + [(None, 15), (None, 16), (None, 270)] + [(m, k) for m in (19, 274) for k in (4, 5, 6)]


def _lz4_block(seqs, tail):
    """an LZ4 block from (literal bytes, offset, match length) triples + the final literals — written by hand so that the
    test chooses every length and alignment itself"""
    out = bytearray()
    def ext(v):
        while v >= 255: out.append(255); v -= 255
        out.append(v)
    for lit, off, m in seqs:
        out.append((min(len(lit), 15) << 4) | min(m - 4, 15))
        if len(lit) >= 15: ext(len(lit) - 15)
        out += lit
        out += bytes((off & 255, off >> 8))
        if m - 4 >= 15: ext(m - 4 - 15)
    out.append(min(len(tail), 15) << 4)
    if len(tail) >= 15: ext(len(tail) - 15)
    out += tail
    return bytes(out)


def _snappy_raw(n, seqs, tail):
    out = bytearray()
    v = n
    while v >= 128: out.append((v & 127) | 128); v >>= 7
    out.append(v)
    def lit(b):
        if not b: return
        k = len(b) - 1
        if k < 60: out.append(k << 2)
        else: out.append(61 << 2); out.extend((k & 255, k >> 8))
        out.extend(b)
    for l, off, m in seqs:
        lit(l)
        while m > 0:                                  # copies of at most 64 bytes, 2-byte offsets
            k = min(m, 64) if m - min(m, 64) == 0 or m - min(m, 64) >= 4 else m - 4
            out.append(((k - 1) << 2) | 2); out.extend((off & 255, off >> 8))
            m -= k
    lit(tail)
    return bytes(out)


def varint(v):
    out = bytearray()
    while v >= 128: out.append((v & 127) | 128); v >>= 7
    out.append(v)
    return bytes(out)


def snappy_elements(seqs, tail, seed):
    """the element stream (no preamble) of the same sequences with every header form: literal headers of 1, 2 and 3 bytes (a length that
    fits a shorter header may use a longer one), copies with 1-, 2- and 4-byte offsets"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    def lit(b):
        if not b: return
        k = len(b) - 1
        form = int(rng.integers(0, 4))                # 0, 1: the shortest header; 2: one length byte; 3: two
        if k >= 256 or form == 3: out.append(61 << 2); out.extend((k & 255, k >> 8))
        elif k >= 60 or form == 2: out.append(60 << 2); out.append(k)
        else: out.append(k << 2)
        out.extend(b)
    for l, off, m in seqs:
        lit(l)
        while m > 0:
            k = min(m, 64) if m - min(m, 64) == 0 or m - min(m, 64) >= 4 else m - 4
            form = int(rng.integers(0, 3))
            if form == 0 and 4 <= k <= 11 and off < 2048: out.append(((off >> 8) << 5) | ((k - 4) << 2) | 1); out.append(off & 255)
            elif form == 2: out.append(((k - 1) << 2) | 3); out.extend(off.to_bytes(4, "little"))
            else: out.append(((k - 1) << 2) | 2); out.extend((off & 255, off >> 8))
            m -= k
    lit(tail)
    return bytes(out)


def sequences(seed, nseq=NSEQ, dict_len=0, middle=False):
    """(literal bytes, offset, match length) x nseq: the first literal is 64 random bytes, then lengths from LITS / MLENS; offsets 1 .. 8
    (overlapping copies), near ones and far ones (up to 65 535 where the chunk is that long, the farthest possible at every 50th
    sequence).  dict_len: the first twenty matches reach into a dictionary of that length (some end in it, some run on into the
    output).  middle: sequence nseq / 2 has 300 literals and a 300-byte match (length extensions of two bytes)."""
    rng = np.random.default_rng(seed)
    seqs, op = [], 0
    for i in range(nseq):
        ll = 64 if i == 0 else int(rng.choice(LITS))
        m = int(rng.choice(MLENS))
        if middle and i == nseq // 2: ll = m = 300
        lit = rng.integers(0, 256, ll, dtype=np.uint8).tobytes()
        op += ll
        kind = int(rng.integers(0, 3))
        if dict_len and i < 20:
            off = op + (int(rng.integers(1, m)) if i % 4 == 0 else int(rng.integers(m, dict_len + 1)) if i % 4 < 3 else dict_len)
        elif i % 50 == 49: off = min(op, 65535)
        elif kind == 0: off = int(rng.integers(1, 9))
        elif kind == 1: off = int(rng.integers(9, 65))
        else: off = int(rng.integers(min(op, 65), min(op, 65535) + 1))
        seqs.append((lit, off, m))
        op += m
    return seqs


def render(seqs, tail, d=b""):
    """the bytes the sequences mean (dictionary d in front of the output) and every sequence's (literal start, match start, match end)"""
    hist = bytearray(d)
    base = len(hist)
    pos = []
    for lit, off, m in seqs:
        ls = len(hist) - base
        hist += lit
        ms = len(hist) - base
        assert 0 < off <= len(hist)
        if off >= m: hist += hist[len(hist) - off:len(hist) - off + m]
        else: hist += (bytes(hist[len(hist) - off:]) * (m // off + 1))[:m]
        pos.append((ls, ms, ms + m))
    hist += tail
    return bytes(hist[base:]), pos


def capacities(U, pos, cuts=CUTS):
    s = set(range(U - 24, U + 25)) | {0, 1, 2, 11, 12, 13}
    for j in cuts:
        for p in pos[j]:
            s |= set(range(p - 2, p + 16))
    return sorted(c for c in s if c >= 0)


def big_capacities(U):
    s = set(range(U - 24, U + 25))
    for b in (32768, 65536, 98304):
        s |= set(range(b - 16, b + 17))
    return sorted(s)


def _ext_bytes(v, base):
    return 0 if v < base else (v - base) // 255 + 1


def _streams(seqs, seed, d=b"", tails=TAILS, cuts=CUTS, caps=capacities):
    """one stream per tail: name, seqs, tail, raw (the intended bytes), U, caps, legal (LZ4: the input-side end rule holds — behind the
    last match's literals at least 8 bytes follow: offset, its length extension, the last token, its extension, the final literals)"""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for m_last, k in tails:
        sq = list(seqs)
        if m_last is not None: sq[-1] = (sq[-1][0], sq[-1][1], m_last)
        tail = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
        raw, pos = render(sq, tail, d)
        legal = 2 + _ext_bytes(sq[-1][2] - 4, 15) + 1 + _ext_bytes(k, 15) + k >= 8
        out.append(dict(name="seed%d/match%s/tail%d" % (seed, m_last, k), seqs=sq, tail=tail, raw=raw, U=len(raw), caps=caps(len(raw), pos) if cuts else caps(len(raw)),
                        legal=legal, final_lits=k))
    return out


# ---- the batches: lists of cases {stream (its name), bytes, cap, U, final_lits, result, out} ------------------------------------------
LZ4_BODIES = ("a", "b", "long")                  # "long" (the 300-byte literal run and match in its middle): 64 KiB window only
_SEEDS = {"a": 11, "b": 12, "long": 13}


@functools.lru_cache(maxsize=None)
def lz4_streams(body, dict_len=0):
    import lz4_dict_model as D
    d = D.dictionary(dict_len) if dict_len else b""
    out = _streams(sequences(_SEEDS[body] + (100 if dict_len else 0), dict_len=dict_len, middle=body == "long"), _SEEDS[body], d)
    for s in out: s["bytes"] = _lz4_block(s["seqs"], s["tail"])
    return out


CORRUPT = -7                                      # CJ_E_CORRUPT: what every refusal of the raw LZ4 oracle (it says -1) means in a batch


def _lz4_raw(blob, cap):
    r, o = oracle.lz4_decompress_raw(blob, cap)
    return (r, o) if r >= 0 else (CORRUPT, b"")


def _case(s, blob, cap, r, o):
    return dict(stream=s["name"], bytes=blob, cap=cap, U=s["U"], final_lits=s["final_lits"], result=int(r), out=o)


@functools.lru_cache(maxsize=None)
def lz4_cases(body):
    """every (stream, capacity) of one body with the oracle's (result, bytes)"""
    return [_case(s, s["bytes"], c, *_lz4_raw(s["bytes"], c)) for s in lz4_streams(body) for c in s["caps"]]


@functools.lru_cache(maxsize=None)
def lz4_dict_cases(body, dict_len=4096):
    import lz4_dict_model as D
    d = D.dictionary(dict_len)
    return [_case(s, s["bytes"], c, *D.decode(s["bytes"], c, d)) for s in lz4_streams(body, dict_len) for c in s["caps"]]


PREFIX_ROOM = 64                                  # the size-prefix sweep: out_cap = U + 64


@functools.lru_cache(maxsize=None)
def lz4_prefix_cases(body):
    """the PREFIX swept over the capacity list (+ a few values above out_cap, negative and too big for any block) under out_cap = U + 64"""
    out = []
    for s in lz4_streams(body):
        room = s["U"] + PREFIX_ROOM
        for v in s["caps"] + [room, room + 1, room + 100, 0x7E000000, 0x7E000001, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]:
            blob = v.to_bytes(4, "little") + s["bytes"]
            out.append(_case(s, blob, room, *oracle.lz4_block_decompress(blob, room, True)))
            out[-1]["prefix"] = v
    return out


@functools.lru_cache(maxsize=None)
def snappy_streams(body):
    out = _streams(sequences(_SEEDS[body] + 50), _SEEDS[body] + 50)
    for s in out: s["elements"] = snappy_elements(s["seqs"], s["tail"], _SEEDS[body])
    return out


SNAPPY_BODIES = ("a", "b")


@functools.lru_cache(maxsize=None)
def snappy_cases(body):
    """pass 1: the preamble declares each value of the capacity list and out_cap is that value; pass 2: the true preamble under
    out_cap = U - 24 .. U + 24"""
    out = []
    for s in snappy_streams(body):
        for c in s["caps"]:
            blob = varint(c) + s["elements"]
            out.append(_case(s, blob, c, *oracle.snappy_decompress(blob, c)))
        blob = varint(s["U"]) + s["elements"]
        for c in range(s["U"] - 24, s["U"] + 25):
            out.append(_case(s, blob, c, *oracle.snappy_decompress(blob, c)))
    return out


@functools.lru_cache(maxsize=None)
def big_streams():
    """one LZ4 and one Snappy stream of ~100 KiB decoded: 3 900 sequences, offsets up to 65 535, 13 final literals"""
    seqs = sequences(21, BIG_NSEQ)
    s = _streams(seqs, 21, tails=[(None, 13)], cuts=None, caps=big_capacities)[0]
    s["bytes"] = _lz4_block(s["seqs"], s["tail"])
    s["elements"] = snappy_elements(s["seqs"], s["tail"], 21)
    return s


@functools.lru_cache(maxsize=None)
def big_cases(codec):
    s = big_streams()
    if codec == "lz4":
        return [_case(s, s["bytes"], c, *_lz4_raw(s["bytes"], c)) for c in s["caps"]]
    return [_case(s, varint(c) + s["elements"], c, *oracle.snappy_decompress(varint(c) + s["elements"], c)) for c in s["caps"]]


def _paths():
    """every LZ4 / Snappy decoder path of a device-resident batch as (flags, window) test parameters: one wavefront / one lane per
    chunk, the workgroup decoder behind the parse kernel and with the parse inside it, the default pipeline, the 32 KiB and 16 KiB
    windows with each placement of the parse"""
    import pytest
    from cramjam_amd import _native as N
    WAVE, LANE, LDS = N.FLAG_FORCE_WAVE_PER_CHUNK, N.FLAG_FORCE_LANE_PER_CHUNK, N.FLAG_FORCE_LDS_PER_CHUNK
    PK, FUSED, LE32, LE16 = N.FLAG_FORCE_PARSE_KERNEL, N.FLAG_FORCE_FUSED_PARSE, N.FLAG_CHUNKS_LE_32K, N.FLAG_CHUNKS_LE_16K
    return [pytest.param(WAVE, 65536, id="wave-per-chunk"), pytest.param(LANE, 65536, id="lane-per-chunk"),
            pytest.param(LDS | PK, 65536, id="lds+parse-kernel"), pytest.param(LDS | FUSED, 65536, id="lds+fused-parse"), pytest.param(0, 65536, id="default"),
            pytest.param(LE32, 32768, id="le32k"), pytest.param(LE32 | PK, 32768, id="le32k+parse-kernel"), pytest.param(LE32 | FUSED, 32768, id="le32k+fused-parse"),
            pytest.param(LE16, 16384, id="le16k"), pytest.param(LE16 | PK, 16384, id="le16k+parse-kernel"), pytest.param(LE16 | FUSED, 16384, id="le16k+fused-parse")]


PATHS = _paths()


def lz4_bodies(win):
    return LZ4_BODIES if win >= 65536 else LZ4_BODIES[:2]              # (the body with the 300-byte runs: 64 KiB window only)


def run_and_check(eng, codec, flags, key, cases, dictionary=None):
    """one device-resident decode batch over a case list on the harness (tests/device_batch.py): the oracle's result and bytes, both
    guards intact — accepted or refused —, [result, cap) untouched where the chunk was accepted; returns (results, output, slot offsets)"""
    import device_batch as DB
    from cramjam_amd import _native as N
    n = len(cases)
    if dictionary is None:
        call = lambda i, o, l, out, oo, oc, r: eng.batch_device(codec, N.OP_DECOMPRESS, flags, n, i, o, l, out, oo, oc, r)
    else:
        call = lambda i, o, l, out, oo, oc, r, d: N.check(N.lib().cj_dict_batch_device(eng.h, codec, N.OP_DECOMPRESS, flags, n, i, o, l, out, oo, oc, r, d, len(dictionary), None))
    tag = lambda i, got: (key, hex(flags), cases[i]["stream"], "cap", cases[i]["cap"], "U", cases[i]["U"], "got", got, "want", cases[i]["result"])
    return DB.run_cases(eng, key, cases, call, tag, dictionary=dictionary)
