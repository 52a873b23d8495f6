"""Mint tests/golden/enc_model_digests.json: the returned length and the SHA-256 of the output of every entry of the scalar encoder
models under tests/hostsim (enc2_model_lz4 / _snappy at three round sizes, enc2_model_lz4_linked at four histories, dfe_model_compress
under its three wrappers, zse_model_compress with and without the checksum) on the seeded inputs of tests/enc_model_digests.py.  The
file pins the models' bytes: it is minted from the models as they stand BEFORE a change to them that must keep every byte, and
tests/test_enc_model_digests.py holds the changed models to it.  Data only.

    python tests/golden/make_enc_model_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import deflate_enc_cases as DE  # noqa: E402
import enc_model_digests as M  # noqa: E402
import zstd_enc_cases as ZE  # noqa: E402


def main():
    # the input where the distance limit decides: DEFLATE keeps the match 32 768 back alone, Zstandard all three
    far = M.far_input()
    want = {d for _, d in M.FAR}
    dfe = {r[2] for r in DE.records(far[:65536]) if r[3] >= 4} & want
    zse = {r[2] for r in ZE.records(far[:65536]) if r[3] >= 4} & want
    assert dfe == {32768} and zse == want, (dfe, zse)
    j = {"inputs": [name for name, _ in M.inputs()], "digests": M.digests()}
    path = os.path.join(HERE, "enc_model_digests.json")
    with open(path, "w") as f:
        json.dump(j, f, indent=0, sort_keys=True)
    print("entries %d, inputs %d, %d bytes" % (len(j["digests"]), len(j["inputs"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
