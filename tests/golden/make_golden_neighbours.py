"""Mint tests/golden/golden_neighbours.json: libzstd's verdict (ctypes; tests/zstd_cases.py) on every cut s[:k] of the six base frames
of tests/neighbour_cases.py (ZSTD_BASES, taken from tests/golden/golden_zstd.bin) at capacities U and U + 64 — per base one list of
results per capacity, and the SHA-256 of the bytes of every accepted cut.  Run from the repository root:
python tests/golden/make_golden_neighbours.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import neighbour_cases as NC  # noqa: E402

if __name__ == "__main__":
    doc = NC.mint_zstd()
    with open(NC.GOLDEN_JSON, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(NC.GOLDEN_JSON, os.path.getsize(NC.GOLDEN_JSON), "bytes;", sum(len(b["results"][0]) for b in doc["bases"]), "cuts;",
          sum(len(b["sha256"]) for b in doc["bases"]), "accepted")
