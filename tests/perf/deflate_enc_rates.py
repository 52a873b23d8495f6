"""Rates and ratios of the DEFLATE batch encoder on one MI355X.  Device-resident, HIP events, a warm-up and the median
of RUNS runs with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/deflate_enc_rates.py [--quick]      (--quick: one pass of every batch at a tenth of the size)
  python tests/perf/deflate_enc_rates.py --python-host  (only the last figure: batch.deflate_compress_many host to host, wall time)
Batches: the corpus's full 64 KiB chunks (bench.py --data corpus64k) tiled to 20 000, bench.py's synth-v1 chunks tiled to 20 000, and
100 000 word-like records of 4 KiB; each as raw DEFLATE and as gzip (the difference is the checksum's cost).
Yardsticks in the same session: zlib levels 1 and 6 on 16 threads over the same payloads (it releases the GIL), and this library's
LZ4 block encoder over the same payloads (the same matcher without the entropy stage)."""
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as D  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9


def say(**kw):
    print(json.dumps(kw), flush=True)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def timed(fn, side):
    ev = []
    for k in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        side.synchronize()
        a.record(side)
        fn()
        b.record(side)
        side.synchronize()
        if k or QUICK:
            ev.append(a.elapsed_time(b))
    return ev


def shape(side, eng, label, uniq, n):
    dev = torch.device("cuda:0")
    L = N.lib()
    S = len(uniq[0])
    reps = max(n // len(uniq), 1)
    n = reps * len(uniq)
    label = "%s: %d x %d B" % (label, n, S)
    s = side.cuda_stream
    p = lambda t: t.data_ptr()
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
    with torch.cuda.stream(side):
        raw = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev).repeat(reps)
        raw = torch.cat([raw, torch.zeros(64, dtype=torch.uint8, device=dev)])
        ioff, ilen = i64(np.arange(n) * S), i64(np.full(n, S))
        res = torch.empty(n, dtype=torch.int64, device=dev)
        back = torch.empty(n * S + 64, dtype=torch.uint8, device=dev)
        res2 = torch.empty(n, dtype=torch.int64, device=dev)
    side.synchronize()
    rates = {}
    for wrap in (D.RAW, D.GZIP):
        stride = (L.cj_deflate_compress_bound(S, wrap) + 15) // 16 * 16
        with torch.cuda.stream(side):
            coff, ccap = i64(np.arange(n) * stride), i64(np.full(n, stride))
            comp = torch.empty(n * stride + 64, dtype=torch.uint8, device=dev)
        ev = timed(lambda: N.check(L.cj_deflate_compress_batch_device(eng.h, wrap, 0, n, p(raw), p(ioff), p(ilen), p(comp), p(coff), p(ccap), p(res), s)), side)
        assert int(res.min()) > 0
        # what was written reads back: this library's decoder over the whole batch, zlib over the first unique streams
        N.check(L.cj_deflate_batch_device(eng.h, wrap, N.OP_DECOMPRESS, 0, n, p(comp), p(coff), p(res), p(back), p(ioff), p(ilen), p(res2), s))
        side.synchronize()
        assert int(res2.min()) == S and int(res2.max()) == S and torch.equal(back[:n * S], raw[:n * S])
        r0 = res[:len(uniq)].cpu().numpy()
        head = comp[:len(uniq) * stride].cpu().numpy()
        for k in range(min(len(uniq), 16)):
            assert zlib.decompress(head[k * stride:k * stride + int(r0[k])].tobytes(), D.WBITS[wrap]) == uniq[k]
        rates[wrap] = statistics.median(ev)
        say(what=label + ": compress, " + D.WRAP_NAME[wrap], GBps=round(n * S / rates[wrap] / 1e6, 2), ratio=round(len(uniq) * S / int(r0.sum()), 3), **stats(ev))
        del comp
    say(what=label + ": checksum's cost (gzip over raw)", times=round(rates[D.GZIP] / rates[D.RAW], 3))
    # yardstick 1: zlib levels 1 and 6 on 16 threads over the same payloads
    for level in (1, 6):
        k = min(n, 16 * max(1, (200 if QUICK else 2000) * 4096 // S // (1 if level == 1 else 4)))

        def work(t):
            total = 0
            for i in range(t, k, 16):
                c = zlib.compressobj(level, zlib.DEFLATED, -15)
                total += len(c.compress(uniq[i % len(uniq)]) + c.flush())
            return total
        ts = []
        with ThreadPoolExecutor(16) as ex:
            for _ in range(RUNS + 1):
                t = time.perf_counter(); sizes = list(ex.map(work, range(16))); ts.append((time.perf_counter() - t) * 1e3)
        cpu = statistics.median(ts[1:] or ts)
        say(what=label + ": yardstick, zlib level %d on 16 threads, raw" % level, payloads=k, GBps=round(k * S / cpu / 1e6, 3), ratio=round(k * S / sum(sizes), 3),
            gpu_over_it=round((n * S / rates[D.RAW]) / (k * S / cpu), 1), **stats(ts[1:] or ts))
    # yardstick 2: this library's LZ4 block encoder over the same payloads
    with torch.cuda.stream(side):
        stride = (L.cj_lz4_block_compress_bound(S, 0) + 15) // 16 * 16
        coff, ccap = i64(np.arange(n) * stride), i64(np.full(n, stride))
        comp = torch.empty(n * stride + 64, dtype=torch.uint8, device=dev)
    ev = timed(lambda: N.check(L.cj_batch_device(eng.h, 0, N.OP_COMPRESS, 0, n, p(raw), p(ioff), p(ilen), p(comp), p(coff), p(ccap), p(res), s)), side)
    lz = statistics.median(ev)
    say(what=label + ": yardstick, LZ4 block encoder over the same payloads", GBps=round(n * S / lz / 1e6, 1), ratio=round(n * S / int(res.sum()), 3),
        deflate_raw_over_it=round(rates[D.RAW] / lz, 2), **stats(ev))


def python_host(uniq, n):
    """batch.deflate_compress_many from host buffers to new `bytes` objects and into one buffer: wall time of the whole Python call"""
    chunks = [uniq[i % len(uniq)] for i in range(n)]
    total = sum(len(c) for c in chunks)
    out = bytearray(sum(batch.deflate_compress_bound(len(c), "gzip") for c in chunks))
    for label, kw in (("new bytes objects", {}), ("into one buffer", {"out": out})):
        ms = []
        for k in range(RUNS + 1):
            t = time.perf_counter()
            res, outs = batch.deflate_compress_many(chunks, wrapper="gzip", **kw)
            if k or QUICK:
                ms.append((time.perf_counter() - t) * 1e3)
        assert min(res) > 0 and all(zlib.decompress(bytes(outs[i]), D.WBITS[D.GZIP]) == chunks[i] for i in range(0, n, max(n // 16, 1)))
        say(what="batch.deflate_compress_many, host to host, gzip, %s: %d x %d B" % (label, n, len(chunks[0])),
            GBps=round(total / statistics.median(ms) / 1e6, 2), **stats(ms))


def main():
    import bench
    import oracle
    corpus, _ = bench.corpus_chunks(65536)
    if "--python-host" in sys.argv:
        return python_host(corpus, 4096 // (10 if QUICK else 1))
    side = torch.cuda.Stream()
    eng = batch._engine(0)
    scale = 10 if QUICK else 1
    shape(side, eng, "corpus64k", corpus, 20000 // scale)
    shape(side, eng, "synth-v1", [oracle.synth_v1(65536, i) for i in range(256)], 20000 // scale)
    shape(side, eng, "text records", [D.words(4096, 9000 + k) for k in range(256)], 100000 // scale)
    python_host(corpus, 4096 // scale)


if __name__ == "__main__":
    main()
