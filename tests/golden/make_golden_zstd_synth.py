"""Writes golden_zstd_synth.json: libzstd's verdicts on the synthesized Zstandard streams of tests/zstd_synth.py and on 600 seeded
single-bit flips of them, for the GPU tests (tests/test_zstd_synth_gpu.py), which do not call libzstd.  The file holds no streams: they
are made again from their seeds, and the recorded digest of each (SHA-256, its first 128 bits) catches a generator that has drifted.
tests/test_zstd_synth_model.py asserts that the file is what the generator and the loaded libzstd say today."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_cases as Z  # noqa: E402
import zstd_synth as S  # noqa: E402


def main():
    entries = S.recorded_entries()
    path = os.path.join(HERE, "golden_zstd_synth.json")
    with open(path, "w") as f:
        f.write('{"libzstd": %s, "cases": [\n' % json.dumps(Z.libzstd().ZSTD_versionString().decode()))
        rows = [json.dumps(e, separators=(",", ":")) for e in entries]
        f.write(",\n".join(",".join(rows[k:k + 5]) for k in range(0, len(rows), 5)))
        f.write("\n]}\n")
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print("%d entries, %d bytes" % (len(entries), os.path.getsize(path)))


if __name__ == "__main__":
    main()
