"""The LZ4 raw-block cases the size-query tests share (tests/test_batch_sizes_model.py on the CPU, tests/batch_sizes_child.py on the
GPU), and the oracle's statement of what the query returns: the length the safe decoder produces when output room never runs out."""
import bz2
import json
import os
import random
from base64 import b64decode

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E_CORRUPT, E_PREFIX_TOO_BIG = -7, -5
OUT_MAX, IN_MAX, SLACK = 0x7E000000, 0x7FFFFFF0, 12

_room = None


def oracle_decode(blob, cap):
    """oracle.lz4_decompress_raw(blob, cap)[0] without a zero-filled buffer of cap bytes per call (cap goes up to gigabytes: the
    pages of one lazily mapped array are only touched where the decoder writes)"""
    global _room
    if _room is None or _room.size < cap:
        _room = None
        _room = np.empty(max(cap, 1 << 20), np.uint8)
    b = np.frombuffer(blob, np.uint8) if len(blob) else np.zeros(1, np.uint8)
    return int(oracle.lib().cjo_lz4_decompress_raw(b.ctypes.data, len(blob), _room.ctypes.data, cap))


def expected_size(blob):
    """what cj_batch_sizes_device answers for a raw LZ4 block, from the oracle alone"""
    if len(blob) > IN_MAX:
        return E_CORRUPT
    s = oracle_decode(blob, 255 * len(blob) + 64)
    return E_CORRUPT if s < 0 else E_PREFIX_TOO_BIG if s > OUT_MAX else s


def huge_match_block():
    """one match that announces more than 0x7E000000 bytes through ~8.3 MB of 0xFF length bytes"""
    nff = OUT_MAX // 255 + 2
    return bytes([0x1F, 0x41, 0x01, 0x00]) + b"\xff" * nff + bytes([7]) + bytes([0x50]) + b"tail!"


def text(n, seed):
    """n bytes of text: the corpus's plain-text files, cut and rejoined at random so that the matches do not line up"""
    rnd = random.Random(seed)
    src = b"".join(bz2.decompress(open(os.path.join(GOLDEN, "corpus", f + ".bz2"), "rb").read()) for f in ("alice29.txt", "asyoulik.txt", "lcet10.txt"))
    out = bytearray()
    while len(out) < n:
        a = rnd.randrange(len(src) - 5000)
        out += src[a:a + rnd.randrange(200, 5000)]
    return bytes(out[:n])


def lz4_cases(big=True):
    """[(tag, block, from_encoder)]: from_encoder = the block came unmodified out of an encoder (it obeys the end-of-block rules)"""
    g = json.load(open(os.path.join(GOLDEN, "golden_vectors.json")))
    cases = [(("golden", v["name"]), b64decode(v["lz4"]), True) for v in g["vectors"]]
    cases += [(("malformed", m["src"], m["kind"], m["k"]), b64decode(m["data"]), False) for m in g["malformed_lz4"]]
    rnd = random.Random(11)
    for t in range(220):
        n = rnd.choice([0, 1, 5, 13, 40, 100, 1000, 5000, 20000, 70000])
        alpha = rnd.choice([2, 3, 4, 16, 64, 256])
        raw = bytes(rnd.choices(range(alpha), k=n))
        if rnd.random() < 0.5 and n > 10:
            raw = (raw[:rnd.randrange(1, 20)] * n)[:n]                 # a repeated prefix: long matches, length bytes
        blob = oracle.lz4_compress_raw(raw)[1]
        cases.append((("fuzz", t), blob, True))
        if len(blob) > 3:
            b = bytearray(blob)
            for _ in range(rnd.randrange(1, 4)):
                b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
            cases.append((("flip", t), bytes(b), False))
            cases.append((("cut", t), blob[:rnd.randrange(len(blob))], False))
    for i in range(6):
        cases.append((("synth", i), oracle.lz4_compress_raw(oracle.synth_v1(65536, i))[1], True))
    cases.append((("text", 300 << 10), oracle.lz4_compress_raw(text(300 << 10, 1))[1], True))
    if big:
        cases.append((("text", 5 << 20), oracle.lz4_compress_raw(text(5 << 20, 2))[1], True))
        cases.append((("huge-match",), huge_match_block(), False))
    return cases
