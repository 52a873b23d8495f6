"""Mint tests/golden/golden_deflate.json + golden_deflate.bin from Python's zlib module (the system zlib): the payload x level x
strategy x wrapper matrix of tests/deflate_cases.py (thinned per payload so that each file stays under 1 MiB), the 300 000-byte text
written with Z_SYNC_FLUSH every 7 000 bytes, seeded single-bit flips and cuts of six of those streams, and zlib's verdict on the
hand-written streams of tests/deflate_cases.py.  Every entry carries the wrapper, where its stream lies in the .bin (mutations: their
base stream and the bit; hand-written streams are rebuilt by deflate_cases.hand_streams), zlib's verdict at its capacity and the
sha256 and length of the output.  Data only.

    python tests/golden/make_golden_deflate.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deflate_cases as D  # noqa: E402

MUTATION_BASES = ("text300_l6_default_raw", "text4k_l6_default_raw", "text4k_l9_default_zlib", "text4k_l1_fixed_raw", "text300_l6_default_gzip",
                  "dist32768_l1_default_raw")
MUTATIONS, SLACK = 600, 1024          # capacity of a mutated stream: its base's length + SLACK (a flip may lengthen the output)


def main():
    blob, valid = bytearray(), []

    def keep(name, wrap, s, raw, **kw):
        r, out = D.verdict(wrap, s, len(raw))
        assert r == len(raw) and out == raw, name
        valid.append(dict(name=name, wrap=wrap, off=len(blob), len=len(s), result=r, n=len(raw), sha256=D.sha(raw), **kw))
        blob.extend(s)

    for pname, raw in D.payloads().items():
        for level, strategy, wrap in D.matrix(pname):
            keep("%s_l%d_%s_%s" % (pname, level, D.STRATEGY_NAME[strategy], D.WRAP_NAME[wrap]), wrap, D.compress(raw, level, strategy, wrap), raw,
                 payload=pname, level=level, strategy=D.STRATEGY_NAME[strategy])
    assert all(name in {v["name"] for v in valid} for name in MUTATION_BASES)
    text = D.flush_text()
    for wrap in (D.RAW, D.GZIP):
        keep("flush300k_%s" % D.WRAP_NAME[wrap], wrap, D.compress_flushed(text, wrap), text, payload="flush300k", level=6, strategy="default")

    by = {v["name"]: v for v in valid}
    g = D._lcg(2024)
    muts = []
    for m in range(MUTATIONS):
        base = by[MUTATION_BASES[m % len(MUTATION_BASES)]]
        s = bytes(blob[base["off"]:base["off"] + base["len"]])
        cut, bit = None, 0
        if m % 25 == 24:
            cut = next(g) % len(s)
            ms = s[:cut]
        else:
            bit = next(g) % (8 * len(s))
            ms = D.flip(s, bit)
        cap = base["n"] + SLACK
        r, out = D.verdict(base["wrap"], ms, cap)
        muts.append(dict(name="mut%03d_%s" % (m, base["name"]), base=base["name"], bit=bit, cut=cut, cap=cap, result=r, n=len(out), sha256=D.sha(out)))
    accepted = sum(1 for m in muts if m["result"] >= 0)
    assert accepted >= 60 and len(muts) - accepted >= 60, accepted

    hand = []
    for name, wrap, s in D.hand_streams():
        cap = 1024
        r, out = D.verdict(wrap, s, cap)
        hand.append(dict(name=name, cap=cap, result=r, n=len(out), sha256=D.sha(out)))

    import zlib
    # compact rows (deflate_cases._load expands them): streams [name = payload_l<level>_<strategy>_<wrapper>, length in the .bin (they lie
    # back to back), n, sha256], mutations [base index, bit, cut, result, n, sha256 or null], hand-written
    # [name, result, n, sha256 or null]; null = no output.  Their capacities are base n + mutation_slack and hand_cap.
    names = [v["name"] for v in valid]
    row = lambda m: [m["result"], m["n"], m["sha256"] if m["n"] else None]
    mrows = [[names.index(m["base"]), m["bit"], m["cut"]] + row(m) for m in muts]
    hrows = [[h["name"]] + row(h) for h in hand]
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    lines = lambda rows, per: ",\n".join(",".join(dumps(r) for r in rows[k:k + per]) for k in range(0, len(rows), per))
    with open(os.path.join(HERE, "golden_deflate.bin"), "wb") as f:
        f.write(blob)
    with open(os.path.join(HERE, "golden_deflate.json"), "w") as f:
        f.write('{"zlib":%s,"mutation_slack":%d,"hand_cap":%d,\n"valid":[\n%s],\n"mutations":[\n%s],\n"hand":[\n%s]}\n'
                % (dumps(zlib.ZLIB_VERSION), SLACK, 1024, lines([[v["name"], v["len"], v["n"], v["sha256"]] for v in valid], 1), lines(mrows, 4), lines(hrows, 6)))
    print("%d streams (%d bytes), %d mutations (%d accepted), %d hand-written (%d accepted)"
          % (len(valid), len(blob), len(muts), accepted, len(hand), sum(1 for h in hand if h["result"] >= 0)))
    assert len(blob) < (1 << 20) and os.path.getsize(os.path.join(HERE, "golden_deflate.json")) < (1 << 20)


if __name__ == "__main__":
    main()
