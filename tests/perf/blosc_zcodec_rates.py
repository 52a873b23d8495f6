"""Times of the Zlib / Zstd reading of Blosc chunks on one MI355X, beside its parts taken in the same run.
Device-resident, HIP events, a warm-up and the median of RUNS runs.  torch is imported first (one HIP runtime per process).  Needs
libblosc (it mints the chunks at run time; nothing of that size is committed).  Prints one JSON line per figure.
  python tests/perf/blosc_zcodec_rates.py [--quick]
Batches: 2 000 x 256 KiB float32 ramp chunks, shuffle: Zstd clevel 5 unsplit (c-blosc's default for it), Zstd always split, Zlib
clevel 5 (split by default).  For each: the Blosc call with its flag; (a) the same non-stored streams as a plain
zstd_decompress_many_device / deflate_decompress_many_device(wrapper="zlib") batch — the decoders' own kernels; (b) the unfilter pass
alone over the same bytes in the chunks' block size (cj_debug_blosc_filter); and the call's time less (a) and (b): the two walk
launches, the one wait with its copy of the counts, the copy of the chunk table, the stored streams' copies and the verdict."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import blosc_zcodec_model as Z  # noqa: E402
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
    ooff = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    want = torch.from_numpy(np.frombuffer(b"".join(plains) * repeat, np.uint8).copy()).to(dev)
    chunks = [G.mint(lib, p, recipe) for p in plains]
    zstd = recipe["cname"] == "zstd"
    assert all(Z.fmt_of(c) == (Z.FORMAT_ZSTD if zstd else Z.FORMAT_ZLIB) for c in chunks)
    blob, coff, clen = DB.pack(chunks * repeat, mis=0, dtype=np.int64)
    res = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.stream(side):
        comp = torch.from_numpy(blob).to(dev)
        back = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        d = [i64(coff), i64(clen), i64(ooff), i64(sizes)]
        ev = timed(lambda: batch.blosc_decompress_chunks_device(comp, d[0], d[1], back, d[2], d[3], result=res, stream=side.cuda_stream, zlib=not zstd, zstd=zstd), side)
        assert torch.equal(res.cpu(), torch.from_numpy(sizes)) and torch.equal(back[:total], want), label
    call = statistics.median(ev)
    h0, s0 = Z.parse(chunks[0])
    say(what=label + ": the Blosc call with its flag", chunks=n, plain_bytes=total, ratio=round(total / float(clen.sum()), 3), blocksize=h0["blocksize"],
        streams_per_chunk=len(s0), GBps=round(total / call / 1e6, 1), **stats(ev))
    # (a) the same streams as a plain batch of the decoder's own
    soff, sln, scap, stored = [], [], [], 0
    for i in range(n):
        for s in Z.parse(chunks[i % len(plains)])[1]:
            if s[5]:
                stored += 1
            else:
                soff.append(int(coff[i]) + s[0]); sln.append(s[1]); scap.append(s[3])
    so = np.concatenate([[0], np.cumsum((np.asarray(scap) + 15) // 16 * 16)[:-1]])
    with torch.cuda.stream(side):
        plain = torch.empty(int(so[-1] + scap[-1]) + 64, dtype=torch.uint8, device=dev)
        r2 = torch.empty(len(soff), dtype=torch.int64, device=dev)
        d2 = [i64(soff), i64(sln), i64(so), i64(scap)]
        if zstd:
            fn = lambda: batch.zstd_decompress_many_device(comp, d2[0], d2[1], plain, d2[2], d2[3], result=r2, stream=side.cuda_stream, sync=False)
        else:
            fn = lambda: batch.deflate_decompress_many_device(comp, d2[0], d2[1], plain, d2[2], d2[3], wrapper="zlib", result=r2, stream=side.cuda_stream, sync=False)
        ev2 = timed(fn, side)
        assert torch.equal(r2.cpu(), torch.from_numpy(np.asarray(scap, np.int64)))
    a_ms = statistics.median(ev2)
    say(what=label + ": (a) the same streams as a plain %s batch" % ("Zstandard" if zstd else "zlib"), streams=len(soff), stored_streams=stored, stream_bytes=sum(scap),
        GBps=round(sum(scap) / a_ms / 1e6, 1), **stats(ev2))
    # (b) the unfilter pass alone: the same number of blocks of the chunks' block size
    eng = batch._engine(0)
    blk = h0["blocksize"]
    nblk = total // blk
    src, dst = eng.alloc(nblk * blk), eng.alloc(nblk * blk)
    N.check(N.lib().cj_memset_dev(eng.h, src, 0x5B, nblk * blk))
    ms, ev3 = C.c_double(0), []
    for k in range(RUNS + 1):
        N.check(N.lib().cj_debug_blosc_filter(eng.h, 0, recipe["filter"], recipe["typesize"], src, dst, blk, blk, nblk, C.byref(ms)))
        if k or QUICK:
            ev3.append(ms.value)
    eng.free(src); eng.free(dst)
    b_ms = statistics.median(ev3)
    say(what=label + ": (b) the unfilter pass alone", blocks=nblk, block=blk, GBps_read_plus_write=round(2 * nblk * blk / b_ms / 1e6, 1), **stats(ev3))
    say(what=label + ": the call less (a) and (b)", call_ms=round(call, 4), a_ms=round(a_ms, 4), b_ms=round(b_ms, 4), rest_ms=round(call - a_ms - b_ms, 4),
        call_over_a=round(call / a_ms, 3))


def main():
    lib = G.load_libblosc()
    if lib is None:
        sys.exit("libblosc.so.1 not found")
    side = torch.cuda.Stream()
    S, uniq = 262144, 50
    ramp = (np.arange(uniq * S // 4, dtype=np.float32) * 0.25).tobytes()
    plains = [ramp[k * S:(k + 1) * S] for k in range(uniq)]
    repeat = 8 if QUICK else 40
    base = dict(clevel=5, filter=1, typesize=4, blocksize=0)
    one_batch(side, lib, "%d x 256 KiB float32 ramp, shuffle, Zstd clevel 5 unsplit" % (uniq * repeat), plains, dict(base, cname="zstd", split=4), repeat)
    one_batch(side, lib, "%d x 256 KiB float32 ramp, shuffle, Zstd clevel 5 always split" % (uniq * repeat), plains, dict(base, cname="zstd", split=1), repeat)
    one_batch(side, lib, "%d x 256 KiB float32 ramp, shuffle, Zlib clevel 5" % (uniq * repeat), plains, dict(base, cname="zlib", split=4), repeat)


if __name__ == "__main__":
    main()
