"""Mint tests/golden/golden_dict.json + golden_dict.bin from the system liblz4: LZ4 blocks written against a dictionary
(LZ4_loadDict + LZ4_compress_fast_continue and, where exported, LZ4_loadDictHC + LZ4_compress_HC_continue), seeded one-byte mutations
of them with the verdict and bytes of LZ4_decompress_safe_usingDict, and that decoder's verdict on the hand-written streams of
tests/lz4_dict_model.py.  Data only; the inputs are regenerated from seeds (lz4_dict_model.record / dictionary).

    python tests/golden/make_golden_dict.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4_dict_model as D  # noqa: E402

MUTATION_BASES = (64, 300, 4096)        # record sizes whose streams are mutated (small streams: a byte is likely to matter)


def main():
    L = D.liblz4()
    assert L is not None, "liblz4 with LZ4_decompress_safe_usingDict is needed to mint the fixtures"
    have_hc = hasattr(L, "LZ4_loadDictHC")
    blob = bytearray()
    valid = []
    for dl in D.DICT_LENS:
        d = D.dictionary(dl)
        for k, size in enumerate(D.RECORD_SIZES):
            raw = D.record(size, k)
            for hc in ((False, True) if have_hc else (False,)):
                s = D.lz4_compress_with_dict(L, raw, d, hc)
                r, out = D.lz4_decode_using_dict(L, s, size, d)
                assert r == size and out == raw
                assert D.decode(s, size, d) == (size, raw), (dl, size, hc)
                assert D.size_walk(s, dl) == size
                valid.append({"name": "d%d_r%d_%s" % (dl, size, "hc" if hc else "fast"), "off": len(blob), "len": len(s), "n": size,
                              "sha256": D.sha(raw), "dict_len": dl, "size": size, "seed": k, "hc": hc})
                blob += s
    # streams that need their dictionary: liblz4 itself refuses them without it
    needs = sum(1 for v in valid if v["n"] >= 64 and D.lz4_decode_using_dict(L, blob[v["off"]:v["off"] + v["len"]], v["n"], b"")[0] < 0)
    assert needs >= len(valid) // 3, needs

    bases = [i for i, v in enumerate(valid) if v["size"] in MUTATION_BASES]
    count, dropped = 300, 0
    while True:
        rng = np.random.default_rng(99)
        muts, dropped = [], 0
        for m in range(count):
            b = bases[int(rng.integers(0, len(bases)))]
            v = valid[b]
            s = bytes(blob[v["off"]:v["off"] + v["len"]])
            pos = int(rng.integers(0, len(s)))
            val = int(rng.integers(0, 256))
            if val == s[pos]:
                val ^= 0x10
            ms = D.mutate(s, pos, val)
            d = D.dictionary(v["dict_len"])
            r, out = D.lz4_decode_using_dict(L, ms, v["n"], d)
            mr, mout = D.decode(ms, v["n"], d)
            agree = (r < 0 and mr == D.CORRUPT) or (r >= 0 and mr == r and mout == out)
            if not agree:
                # the documented deviation (1): liblz4 reads a match of offset 0, this library refuses it
                assert D.has_offset0(ms, v["n"], d), (v["name"], pos, val, r, mr)
                dropped += 1
                continue
            muts.append({"name": "m%03d_%s_p%d" % (m, v["name"], pos), "base": b, "pos": pos, "val": val, "result": r if r >= 0 else D.CORRUPT,
                         "sha256": D.sha(out) if r >= 0 else None})
        ok = sum(1 for m in muts if m["result"] >= 0)
        if ok >= 50 and len(muts) - ok >= 50 and len(muts) >= 300:
            break
        count += 50
    hand = []
    for name, s, cap, dl, accepted in D.hand_streams():
        d = D.dictionary(dl)
        r, out = D.lz4_decode_using_dict(L, s, cap, d)
        mr, mout = D.decode(s, cap, d)
        assert (mr >= 0) == accepted, (name, mr)
        if name == "offset_0":
            assert mr == D.CORRUPT
        else:
            assert (r >= 0) == accepted and (r < 0 or (r == mr and out == mout)), (name, r, mr)
        hand.append({"name": name, "liblz4": r, "result": mr, "sha256": D.sha(mout) if mr >= 0 else None})
    j = {"liblz4_version": int(L.LZ4_versionNumber()), "have_hc": have_hc, "valid": valid, "mutations": muts, "mutations_tried": count,
         "mutations_dropped_offset0": dropped, "hand": hand, "needs_dictionary": needs}
    with open(os.path.join(HERE, "golden_dict.json"), "w") as f:
        json.dump(j, f, indent=0, sort_keys=True)
    with open(os.path.join(HERE, "golden_dict.bin"), "wb") as f:
        f.write(blob)
    print("valid %d (need their dictionary: %d), mutations %d (accepted %d, dropped for offset 0: %d), hand %d, bin %d bytes" %
          (len(valid), needs, len(muts), sum(1 for m in muts if m["result"] >= 0), dropped, len(hand), len(blob)))
    assert len(blob) < (1 << 20) and os.path.getsize(os.path.join(HERE, "golden_dict.json")) < (1 << 20)


if __name__ == "__main__":
    main()
