"""Rates of the BloscLZ reading of Blosc chunks on one MI355X, beside three yardsticks taken in the same run.
Device-resident, HIP events, a warm-up and the median of RUNS runs.  torch is imported first (one HIP runtime per process).  Needs
libblosc (it mints the chunks).  Prints one JSON line per figure.
  python tests/perf/blosclz_rates.py [--quick]
Batches: 10 000 x 256 KiB float32 ramp chunks, shuffle, clevel 5; 2 000 chunks cut from tests/golden/corpus, typesize 1, no filter.
Each as (a) BloscLZ chunks through blosc_decompress_chunks_device(blosclz=True); (1) the same plain bytes as libblosc lz4 chunks
through the same call without the flag; (2) those LZ4 streams through the one-wavefront lz4 kernel (a block batch with
FLAG_FORCE_WAVE_PER_CHUNK: the like-for-like kernel); (3) blosc_decompress_ctx of the BloscLZ chunks on 16 threads.
Yardstick 2 names the kernel with the force flag rather than leaving the size flags off: without any flag the engine routes a batch
of this size to the workgroup decoder (parse + LDS kernels), not to lz4_decode_kernel; the flag is what reaches it at every size."""
import bz2
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import blosc_model as M  # noqa: E402
import device_batch as DB  # noqa: E402
import make_golden_blosc as G  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9


def say(**kw):
    print(json.dumps(kw), flush=True)


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


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def one_batch(side, lib, label, plains, recipe, repeat):
    """plains: the unique plain chunks (bytes); the batch is them `repeat` times over"""
    dev = "cuda"
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
    n = len(plains) * repeat
    sizes = np.asarray([len(p) for p in plains] * repeat)
    total = int(sizes.sum())
    ooff = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]])
    want = torch.zeros(int(ooff[-1] + sizes[-1]) + 64, dtype=torch.uint8, device=dev)
    for i in range(len(plains)):                                    # the expected image of one repeat ...
        want[int(ooff[i]):int(ooff[i]) + len(plains[i])] = torch.from_numpy(np.frombuffer(plains[i], np.uint8).copy()).to(dev)
    first = int(ooff[len(plains) - 1] + sizes[len(plains) - 1])
    for r in range(1, repeat):                                      # ... and every other one behind it: the whole output is compared
        at = int(ooff[r * len(plains)])
        want[at:at + first] = want[:first]
    rates = {}
    for cname, flag in (("blosclz", True), ("lz4", False)):
        chunks = [G.mint(lib, p, dict(recipe, cname=cname)) for p in plains]
        blob, coff, clen = DB.pack(chunks * repeat, mis=0, dtype=np.int64)
        res = torch.empty(n, dtype=torch.int64, device=dev)
        with torch.cuda.stream(side):
            comp = torch.from_numpy(blob).to(dev)
            back = torch.zeros_like(want)
            d = [i64(coff), i64(clen), i64(ooff), i64(sizes)]
            ev = timed(lambda: batch.blosc_decompress_chunks_device(comp, d[0], d[1], back, d[2], d[3], result=res, stream=side.cuda_stream, blosclz=flag), side)
            assert torch.equal(res.cpu(), torch.from_numpy(sizes)) and torch.equal(back, want), cname
        ms = statistics.median(ev)
        rates[cname] = total / ms / 1e6
        say(what="%s: libblosc %s clevel %d chunks, blosc call%s" % (label, cname, recipe["clevel"], " with the flag" if flag else " (yardstick 1)"), chunks=n,
            plain_bytes=total, ratio=round(total / float(clen.sum()), 3), GBps=round(rates[cname], 1), **stats(ev))
        if cname == "lz4":                                           # yardstick 2: the same LZ4 streams, one wavefront per stream
            soff, sln, scap = [], [], []
            for i in range(n):
                for s in M.parse(chunks[i % len(plains)])[1]:
                    if not s[5]:
                        soff.append(int(coff[i]) + s[0]); sln.append(s[1]); scap.append(s[3])
            so = np.concatenate([[0], np.cumsum((np.asarray(scap) + 15) // 16 * 16)[:-1]])
            with torch.cuda.stream(side):
                plain = torch.empty(int(so[-1] + scap[-1]) + 64, dtype=torch.uint8, device=dev)
                r2 = torch.empty(len(soff), dtype=torch.int64, device=dev)
                d2 = [i64(soff), i64(sln), i64(so), i64(scap)]
                p_in, p_out = comp.data_ptr(), plain.data_ptr()
                eng = batch._engine(0)
                ev2 = timed(lambda: eng.batch_device(N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, N.FLAG_FORCE_WAVE_PER_CHUNK, len(soff), p_in, d2[0].data_ptr(), d2[1].data_ptr(),
                                                     p_out, d2[2].data_ptr(), d2[3].data_ptr(), r2.data_ptr(), side.cuda_stream), side)
                assert torch.equal(r2.cpu(), torch.from_numpy(np.asarray(scap, np.int64)))
            rates["wave"] = sum(scap) / statistics.median(ev2) / 1e6
            say(what=label + ": the same LZ4 streams, one wavefront per stream (yardstick 2)", streams=len(soff), stream_bytes=sum(scap), GBps=round(rates["wave"], 1), **stats(ev2))
        else:
            k = min(n, 2000)
            out = C.create_string_buffer(int(sizes.max()))
            t = time.perf_counter()
            for i in range(k):
                assert lib.blosc_decompress_ctx(chunks[i % len(plains)], out, int(sizes[i]), 16) == sizes[i]
            rates["cpu"] = float(sizes[:k].sum()) / (time.perf_counter() - t) / 1e9
            say(what=label + ": blosc_decompress_ctx of the BloscLZ chunks, 16 threads (yardstick 3)", chunks=k, GBps=round(rates["cpu"], 2))
    say(what=label + ": ratios", blosclz_over_lz4_call=round(rates["blosclz"] / rates["lz4"], 3), blosclz_over_wave_kernel=round(rates["blosclz"] / rates["wave"], 3),
        blosclz_over_cpu16=round(rates["blosclz"] / rates["cpu"], 2))


def main():
    lib = G.load_libblosc()
    if lib is None:
        sys.exit("libblosc.so.1 not found")
    side = torch.cuda.Stream()
    S, uniq = 262144, 50
    ramp = (np.arange(uniq * S // 4, dtype=np.float32) * 0.25).tobytes()
    one_batch(side, lib, "10 000 x 256 KiB float32 ramp, shuffle", [ramp[k * S:(k + 1) * S] for k in range(uniq)],
              dict(clevel=5, filter=1, typesize=4, blocksize=0, split=4), (40 if QUICK else 200))
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*")))
    data = b"".join(bz2.decompress(open(f, "rb").read()) for f in files if f.endswith(".bz2"))
    cut = 65536
    pieces = [data[k:k + cut] for k in range(0, len(data) - cut + 1, cut)][:200]
    assert pieces, "tests/golden/corpus holds no data"
    rep = max(1, 2000 // len(pieces))
    one_batch(side, lib, "%d x 64 KiB corpus chunks, typesize 1, no filter" % (len(pieces) * rep), pieces, dict(clevel=5, filter=0, typesize=1, blocksize=0, split=4), rep)


if __name__ == "__main__":
    main()
