"""Mint tests/golden/golden_zstd.json / .bin: Zstandard chunks with the verdicts of the libzstd on this machine (ctypes; see
tests/zstd_cases.py).  Every case records ZSTD_decompress's result at four capacities (cap, cap + 64, cap - 1, 0) and the SHA-256 of
the bytes; the script classifies each chunk by its block and section headers and ASSERTS the coverage matrix, so a fixture set that
misses a mode cannot be written.  Run from the repository root: python tests/golden/make_golden_zstd.py"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_cases as Z  # noqa: E402


def text(n, seed=0):
    src = open(os.path.join(HERE, "plaintext.txt"), "rb").read()
    rnd = random.Random(seed)
    words = src.split()
    out = bytearray(src[:n])
    while len(out) < n:                                       # more text than the file holds: its words in a seeded order
        out += b" ".join(rnd.choice(words) for _ in range(64)) + b"\n"
    return bytes(out[:n])


def rand(n, seed, alphabet=256):
    rnd = random.Random(seed)
    return bytes(rnd.randrange(alphabet) for _ in range(n))


def records(n, seed):
    """4 fresh bytes + 12 constant ones: the same literal length, match length and (repeat) offset in every sequence"""
    rnd = random.Random(seed)
    return b"".join(bytes(rnd.randrange(256) for _ in range(4)) + b"constant-12b" for _ in range(n))


def recipes():
    t = text(300000)
    html = b"".join(b"<tr><td class=\"c%d\">%d</td><td>%s</td></tr>\n" % (i % 7, i * 37, t[i * 11:i * 11 + 9]) for i in range(2000))
    yield "empty_payload", b"", dict(level=3)
    yield "random_1k", rand(1000, 1), dict(level=3)
    yield "zeros_5k", bytes(5000), dict(level=3, checksum=1)
    yield "zeros_300k", bytes(300000), dict(level=3)
    yield "period7", b"abcdefg" * 400, dict(level=3)
    yield "text_300", t[:300], dict(level=3, checksum=1)
    yield "text_4k", t[:4096], dict(level=3)
    yield "text_4k_nofcs", t[:4096], dict(level=1, contentSize=0, checksum=1)
    yield "text_64k", t[:65536], dict(level=3, checksum=1)
    yield "text_150k_l1", t[:150000], dict(level=1, checksum=1)
    yield "text_150k_l19", t[:150000], dict(level=19)
    yield "text_136k_fast", t[:136000], dict(level=-5, contentSize=0)
    yield "mixed_300k", (t[:120000] + rand(20000, 2) + bytes(60000) + html)[:300000], dict(level=3, checksum=1)
    yield "small_alphabet", rand(1500, 3, 4), dict(level=3)
    yield "alphabet16", rand(200, 4, 16), dict(level=3, checksum=1)
    yield "records", records(200, 5), dict(level=3)
    yield "records_l19", records(200, 6), dict(level=19, checksum=1)
    yield "text_tcb", t[:6000], dict(level=3, targetCBlockSize=800, checksum=1)
    yield "html_l9", html[:90000], dict(level=9)
    # 4-stream literals that libzstd decodes with its DOUBLE-symbol Huffman decoder (long and well compressed), no checksum, no content size
    yield "td_rows_l7", b"".join(b"<td>%d</td>\n" % (i * 37) for i in range(6000)), dict(level=7, contentSize=0)


def main():
    L = Z.libzstd()
    print("libzstd", L.ZSTD_versionString().decode())
    named = []                                               # (name, stream, capacity)
    streams = {}
    for name, payload, params in recipes():
        try:
            s = Z.zstd_compress(payload, **params)
        except ValueError as e:
            print("skipped", name, e)
            continue
        streams[name] = s
        named.append((name, s, len(payload)))
    for name, (s, data) in Z.hand_streams().items():
        named.append((name, s, len(data) if data is not None else 64))
        if data is not None:
            r, out = Z.zstd_verdict(s, len(data))
            assert r == len(data) and out == data, (name, r)
    skip = b"\x5a\x2a\x4d\x18" + struct.pack("<I", 5) + b"skip!"
    a, b = streams["text_300"], streams["period7"]
    named.append(("empty", b"", 0))
    named.append(("two_frames", a + b, 300 + 2800))
    named.append(("skippable_everywhere", skip + a + skip + b + skip, 300 + 2800))
    named.append(("skippable_only", skip, 0))
    named.append(("trailing_garbage", a + b"\x00\x01\x02", 300))
    named.append(("bad_magic_behind", a + b"\x00" * 16, 300))
    named.append(("legacy_v07", b"\x27\xb5\x2f\xfd" + a[4:], 300))
    named.append(("dictionary_id", a[:4] + bytes([a[4] | 1]) + a[5:6] + b"\x07" + a[6:], 300))
    named.append(("cut_checksum", a[:-1], 300))
    bases = ["text_300", "text_4k_nofcs", "small_alphabet", "records", "hand_rle_repeat", "td_rows_l7"]
    bases = [(n, dict((x[0], x) for x in named)[n]) for n in bases]
    for k in range(600):
        bn, (_, s, cap) = bases[k % 6]
        named.append(("mut_%03d_%s" % (k, bn), Z.mutate(s, k), cap))
    base_of = dict(("mut_%03d_%s" % (k, bases[k % 6][0]), bases[k % 6]) for k in range(600))

    cases, blob, cover, n_ok, n_bad = [], bytearray(), set(), 0, 0
    for name, s, cap in named:
        verdicts, digest = [], ""
        for c in Z.capacities(cap):
            r, out = Z.zstd_verdict(s, c)
            verdicts.append(r)
            if c == cap and r >= 0:
                digest = Z.sha(out)
        tags = []
        if verdicts[0] >= 0 and not name.startswith("mut_"):
            tags = sorted(Z.classify(s))
            cover |= set(tags)
        if name.startswith("mut_"):
            n_ok += verdicts[0] >= 0
            n_bad += verdicts[0] < 0
        if name in base_of:                                  # stored as an edit of its base: the bytes between a common head and tail
            bn, (_, b, _) = base_of[name]
            pre = next((i for i in range(min(len(b), len(s))) if b[i] != s[i]), min(len(b), len(s)))
            suf = next((i for i in range(min(len(b), len(s)) - pre) if b[len(b) - 1 - i] != s[len(s) - 1 - i]), min(len(b), len(s)) - pre)
            assert b[:pre] + s[pre:len(s) - suf] + b[len(b) - suf:] == s
            cases.append(dict(name=name, base=bn, pre=pre, suf=suf, mid=s[pre:len(s) - suf].hex(), cap=cap, verdicts=verdicts, sha=digest, tags=tags))
            continue
        cases.append(dict(name=name, off=len(blob), len=len(s), cap=cap, verdicts=verdicts, sha=digest, tags=tags))
        blob += s
    missing = [c for c in Z.COVERAGE if c not in cover]
    print("cases", len(cases), "bytes", len(blob), "mutations accepted", n_ok, "refused", n_bad)
    assert not missing, "the fixture set shows no %s" % missing
    assert n_ok >= 60 and n_bad >= 60
    assert len(blob) <= 890 * 1024
    json.dump(dict(libzstd=L.ZSTD_versionString().decode(), cases=cases), open(Z.GOLDEN_JSON, "w"), indent=0)
    open(Z.GOLDEN_BIN, "wb").write(blob)


if __name__ == "__main__":
    main()
