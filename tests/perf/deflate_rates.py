"""Rates of the DEFLATE batch decoder on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS
runs with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/deflate_rates.py [--quick]      (--quick: one pass of every batch at a tenth of the size, for a kernel trace)
Payloads, each compressed with zlib level 6 as raw DEFLATE and as gzip (the difference is the checksum's cost):
  the corpus's full 64 KiB chunks (bench.py --data corpus64k) tiled to 100 000, bench.py's synth-v1 chunks tiled to 100 000, and
  400 000 word-like records of 4 KiB.
Yardsticks in the same session: zlib on 16 threads over the same streams (it releases the GIL), and this library's LZ4 decode of the
same payloads with CJ_FLAG_FORCE_WAVE_PER_CHUNK (the same kernel shape without an entropy stage: the ceiling of this mapping)."""
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


def pack(streams, reps, dev):
    """the unique streams packed 16 bytes apart and repeated reps times at distinct addresses: (blob, off, len) on the device"""
    ln = np.array([len(s) for s in streams], np.int64)
    off = np.concatenate([[0], np.cumsum((ln + 31) & ~15)[:-1]]).astype(np.int64)
    span = int(off[-1] + ((ln[-1] + 31) & ~15))
    buf = np.zeros(span, np.uint8)
    for o, s in zip(off, streams):
        buf[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
    blob = torch.from_numpy(buf).to(dev).repeat(reps)
    offs = (np.arange(reps, dtype=np.int64)[:, None] * span + off[None, :]).reshape(-1)
    return torch.cat([blob, torch.zeros(64, dtype=torch.uint8, device=dev)]), torch.as_tensor(offs, device=dev), torch.as_tensor(np.tile(ln, reps), device=dev)


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
        raw_u = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        ooff, ocap = i64(np.arange(n) * S), i64(np.full(n, S))
        out = torch.empty(n * S + 64, dtype=torch.uint8, device=dev)
        res = torch.empty(n, dtype=torch.int64, device=dev)
    side.synchronize()

    def check():
        assert int(res.min()) == S and int(res.max()) == S
        assert torch.equal(out[:len(uniq) * S], raw_u) and torch.equal(out[(n - len(uniq)) * S:n * S], raw_u)
        out.zero_()

    rates = {}
    for wrap in (D.RAW, D.GZIP):
        streams = [D.compress(u, 6, zlib.Z_DEFAULT_STRATEGY, wrap) for u in uniq]
        with torch.cuda.stream(side):
            blob, off, ln = pack(streams, reps, dev)
        ev = timed(lambda: N.check(L.cj_deflate_batch_device(eng.h, wrap, N.OP_DECOMPRESS, 0, n, p(blob), p(off), p(ln), p(out), p(ooff), p(ocap), p(res), s)), side)
        check()
        rates[wrap] = statistics.median(ev)
        say(what=label + ": decode, " + D.WRAP_NAME[wrap], GBps=round(n * S / rates[wrap] / 1e6, 1), ratio=round(len(uniq) * S / sum(map(len, streams)), 3), **stats(ev))
        if wrap == D.RAW:
            ev = timed(lambda: N.check(L.cj_deflate_batch_sizes_device(eng.h, wrap, 0, n, p(blob), p(off), p(ln), p(res), s)), side)
            assert int(res.min()) == S
            say(what=label + ": size query, raw", GBps_of_output=round(n * S / statistics.median(ev) / 1e6, 1), **stats(ev))
            # yardstick 1: zlib on 16 threads over the same streams
            k = min(n, 16 * max(1, (4000 if QUICK else 40000) * 4096 // S // 16))
            work = lambda t: [zlib.decompress(streams[i % len(streams)], -15) for i in range(t, k, 16)]
            ts = []
            with ThreadPoolExecutor(16) as ex:
                for _ in range(RUNS + 1):
                    t = time.perf_counter(); list(ex.map(work, range(16))); ts.append((time.perf_counter() - t) * 1e3)
            cpu = statistics.median(ts[1:] or ts)
            say(what=label + ": yardstick, zlib inflate on 16 threads, raw", streams=k, GBps=round(k * S / cpu / 1e6, 2), gpu_over_it=round((n * S / rates[wrap]) / (k * S / cpu), 1), **stats(ts[1:] or ts))
        del blob
    say(what=label + ": checksum's cost (gzip over raw)", times=round(rates[D.GZIP] / rates[D.RAW], 3))
    # yardstick 2: LZ4 blocks of the same payloads, one wavefront per chunk
    with torch.cuda.stream(side):
        raw = raw_u.repeat(reps)
        bound = L.cj_lz4_block_compress_bound(S, 0)
        stride = (bound + 15) // 16 * 16
        coff, ccap = i64(np.arange(n) * stride), i64(np.full(n, stride))
        comp = torch.empty(n * stride + 64, dtype=torch.uint8, device=dev)
        cres = torch.empty(n, dtype=torch.int64, device=dev)
        N.check(L.cj_batch_device(eng.h, 0, N.OP_COMPRESS, 0, n, p(raw), p(ooff), p(ocap), p(comp), p(coff), p(ccap), p(cres), s))
    side.synchronize()
    del raw
    ev = timed(lambda: N.check(L.cj_batch_device(eng.h, 0, N.OP_DECOMPRESS, N.FLAG_FORCE_WAVE_PER_CHUNK, n, p(comp), p(coff), p(cres), p(out), p(ooff), p(ocap), p(res), s)), side)
    check()
    lz = statistics.median(ev)
    say(what=label + ": yardstick, LZ4 blocks of the same payloads, CJ_FLAG_FORCE_WAVE_PER_CHUNK", GBps=round(n * S / lz / 1e6, 1), lz4_ratio=round(n * S / int(cres.sum()), 3),
        deflate_raw_over_it=round(rates[D.RAW] / lz, 2), **stats(ev))


def main():
    import bench
    import oracle
    side = torch.cuda.Stream()
    eng = batch._engine(0)
    scale = 10 if QUICK else 1
    corpus, _ = bench.corpus_chunks(65536)
    shape(side, eng, "corpus64k", corpus, 100000 // scale)
    shape(side, eng, "synth-v1", [oracle.synth_v1(65536, i) for i in range(256)], 100000 // scale)
    shape(side, eng, "text records", [D.words(4096, 9000 + k) for k in range(256)], 400000 // scale)


if __name__ == "__main__":
    main()
