"""Wall-clock rate of cj_zstd_compress_batch_device on device-resident chunks: the corpus of tests/golden/corpus as
64 KiB chunks, eight times over, with and without the checksum, and 16 384 word-like records of 4 KiB; a warm-up and the median of five
runs around one enqueue and one synchronisation, one JSON line a batch.  Small batches and a host clock: provisional figures.
    python tests/perf/zstd_enc_rates.py"""
import os, sys, time, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import zstd_enc_cases as E
from cramjam_amd import _native as N
from cramjam_amd.batch import _engine

def run(name, chunks, reps, flags):
    e = _engine(0); L = N.lib()
    n = len(chunks) * reps
    ln = np.array([len(c) for c in chunks] * reps, np.uint64)
    off = np.concatenate([[0], np.cumsum((ln + 31) & ~np.uint64(15))[:-1]]).astype(np.uint64)
    blob = np.zeros(int(off[-1] + ln[-1]) + 64, np.uint8)
    for k in range(n):
        c = chunks[k % len(chunks)]
        blob[int(off[k]):int(off[k]) + len(c)] = np.frombuffer(c, np.uint8)
    cap = np.array([L.cj_zstd_compress_bound(int(x), flags) for x in ln], np.uint64)
    ooff = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.uint64)
    d_in, d_out = e.alloc(blob.nbytes), e.alloc(int(cap.sum()) + 64)
    metas = [e.alloc(8 * n) for _ in range(5)]
    for p, a in zip(metas, (off, ln, ooff, cap)):
        e.h2d(p, a)
    e.h2d(d_in, blob); e.sync()
    ts = []
    for _ in range(6):
        t = time.perf_counter()
        N.check(L.cj_zstd_compress_batch_device(e.h, 0, flags, n, d_in, metas[0], metas[1], d_out, metas[2], metas[3], metas[4], None))
        e.sync()
        ts.append(time.perf_counter() - t)
    res = e.d2h(metas[4], 8 * n, "int64")
    assert (res > 0).all()
    best = sorted(ts[1:])[len(ts[1:]) // 2]
    print(json.dumps({"batch": name, "chunks": n, "flags": flags, "in_bytes": int(ln.sum()), "out_bytes": int(res.sum()), "ratio": float(ln.sum()) / float(res.sum()),
                      "median_ms": 1e3 * best, "GBps_in": float(ln.sum()) / best / 1e9, "all_ms": [1e3 * x for x in ts]}), flush=True)
    for p in [d_in, d_out] + metas:
        e.free(p)

corpus = [c for f in E.corpus_files() for c in E.corpus_chunks(f)]
run("corpus 64KiB", corpus, 8, 0)
run("corpus 64KiB +checksum", corpus, 8, 1)
import deflate_cases as D
recs = [D.words(4096, 500 + i) for i in range(64)]
run("words 4KiB", recs, 256, 0)
