"""Linked against independent LZ4 frame COMPRESSION: rate and ratio through the C-ABI (cj_lz4_frame_compress /
cj_lz4_frame_compress_linked) and through Python (lz4.compress / lz4.Compressor(block_linked=True)), on the reference's corpus and on
64 / 512 MiB of benchmark data (synth-v1); then one large batch of 64 KiB blocks through the batch kernel, independent and linked, for
a kernel trace:
    python tests/perf/linked_frame_compress_rates.py [--sizes-mib 64,512] [--batch-blocks 25000] [--only-batch]
    rocprofv3 --kernel-trace --stats -d OUT -- python tests/perf/linked_frame_compress_rates.py --only-batch
Prints one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
import cramjam_amd as cramjam  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        t.append(time.perf_counter() - t0)
    return min(t), r


def cabi(data, linked, reps):
    L = N.lib()
    cap = L.cj_lz4_frame_compress_bound(len(data))
    out = C.create_string_buffer(cap)
    f = L.cj_lz4_frame_compress_linked if linked else L.cj_lz4_frame_compress
    t, r = best(lambda: f(data, len(data), out, cap, 4), reps)
    assert r > 0, r
    return t, r


def python(data, linked, reps):
    def run():
        if not linked:
            return len(cramjam.lz4.compress(data))
        c = cramjam.lz4.Compressor(block_linked=True)
        c.compress(data)
        return len(c.finish())
    return best(run, reps)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_data(mib):
    return b"".join(oracle.synth_v1(65536, i) for i in range(mib * 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes-mib", default="64,512")
    ap.add_argument("--batch-blocks", type=int, default=25000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-batch", action="store_true")
    a = ap.parse_args()
    if not a.only_batch:
        from test_enc2_linked_model import corpus_streams
        cabi(b"warm" * 100000, True, 1)
        tot = {False: [0, 0, 0.0], True: [0, 0, 0.0]}
        for name, data in corpus_streams():
            row = {"what": "corpus_file", "file": name, "bytes": len(data)}
            for linked in (False, True):
                t, r = cabi(data, linked, a.reps)
                row["linked" if linked else "independent"] = {"ratio": round(len(data) / r, 4), "GBps": round(len(data) / t / 1e9, 3)}
                tot[linked][0] += len(data); tot[linked][1] += r; tot[linked][2] += t
            emit(**row)
        emit(what="corpus_total", **{("linked" if k else "independent"): {"ratio": round(v[0] / v[1], 4), "GBps": round(v[0] / v[2] / 1e9, 3)}
                                     for k, v in tot.items()})
        for mib in [int(x) for x in a.sizes_mib.split(",") if x]:
            data = bench_data(mib)
            for path, fn in (("cabi", cabi), ("python", python)):
                row = {"what": "bench_data", "MiB": mib, "path": path}
                for linked in (False, True):
                    t, r = fn(data, linked, a.reps)
                    row["linked" if linked else "independent"] = {"ratio": round(len(data) / r, 4), "GBps": round(len(data) / t / 1e9, 3)}
                emit(**row)
            del data
    # one batch of 64 KiB blocks through the batch kernel: independent (cj_lz4_frame_compress_blocks above 32 MiB) and linked
    L = N.lib()
    uniq = b"".join(oracle.synth_v1(65536, i) for i in range(64))
    nb = a.batch_blocks
    data = uniq * (nb // 64) + uniq[:65536 * (nb % 64)]
    cap = len(data) + 4 * nb + 16
    out = C.create_string_buffer(cap)
    for linked in (False, True):
        def run():
            if linked:
                return L.cj_lz4_frame_compress_blocks_linked(None, 0, data, len(data), out, cap)
            return L.cj_lz4_frame_compress_blocks(data, len(data), out, cap)
        t, r = best(run, 2)
        assert r > 0, r
        emit(what="batch", blocks=nb, linked=linked, ratio=round(len(data) / r, 4), call_s=round(t, 4))


if __name__ == "__main__":
    main()
