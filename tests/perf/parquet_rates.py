"""Rates of the Parquet chunk batches on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS runs
with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/parquet_rates.py [--quick] [snappy gzip zstd lz4_raw]      (--quick: one pass at a sixteenth of the size)
Per codec, over the benchmark corpus (tests/golden/corpus) cut into pages of about 64 KiB and about 1 MiB, each compressed by this
library's encoders and framed by the model's header writer (tests/parquet_model.py) as V1 pages with CRCs, 16 pages a chunk, repeated
to about TOTAL bytes:
  the decode; the decode with CRC verification; the size query alone; the plain batch of the same page bodies pre-split with known
  lengths (the container's yardstick: what a caller who had parsed every header on the host would run); and the CRC pass's own rate,
  the difference of the two decodes — one wavefront per page, so 1 MiB pages show what splitting a page over wavefronts would buy."""
import bz2
import glob
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
import parquet_model as M  # noqa: E402
import cramjam_amd as cj  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9
TOTAL = (256 << 20) // (16 if QUICK else 1)
PER_CHUNK = 16
dev = torch.device("cuda:0")


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


def i64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)


def corpus_pages(size):
    data = b"".join(bz2.decompress(open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*.bz2"))))
    return [data[i:i + size] for i in range(0, len(data) - size + 1, size)]


def compress(codec, pages):
    """the page bodies, by this library's encoders: the batch encoders, or for LZ4 and Snappy pages above 64 KiB the single-buffer ones"""
    if codec == "gzip":
        res, outs = batch.deflate_compress_many(pages, wrapper="gzip")
    elif codec == "zstd":
        res, outs = batch.zstd_compress_many(pages)
    elif len(pages[0]) > 65536:
        outs = [cj.lz4.compress_block(p, store_size=False) if codec == "lz4_raw" else cj.snappy.compress_raw(p) for p in pages]
        res = [len(bytes(o)) for o in outs]
    elif codec == "lz4_raw":
        res, outs = batch.lz4_compress_blocks(pages, store_size=False)
    else:
        res, outs = batch.snappy_compress_raw_many(pages)
    assert min(res) > 0
    return [bytes(o) for o in outs]


PLAIN_DECODE = {
    "gzip": lambda *a, **kw: batch.deflate_decompress_many_device(*a, wrapper="gzip", **kw),
    "snappy": batch.snappy_decompress_raw_many_device,
    "lz4_raw": lambda *a, **kw: batch.lz4_decompress_blocks_device(*a, store_size=False, **kw),
    "zstd": batch.zstd_decompress_many_device,
}


def one(codec, size, side):
    kw = dict(stream=side.cuda_stream, sync=False)
    uniq = corpus_pages(size)
    bodies = compress(codec, uniq)
    framed = [M.page(b, len(p)) for b, p in zip(bodies, uniq)]
    heads = [len(f) - len(b) for f, b in zip(framed, bodies)]
    npages = max(PER_CHUNK, TOTAL // size // PER_CHUNK * PER_CHUNK)
    order = [k % len(uniq) for k in range(npages)]
    blob = b"".join(framed[k] for k in order)
    ends = np.cumsum([len(framed[k]) for k in order])
    starts = ends - np.array([len(framed[k]) for k in order])
    nch, total = npages // PER_CHUNK, npages * size
    with torch.cuda.stream(side):
        comp = torch.from_numpy(np.frombuffer(blob + bytes(64), np.uint8).copy()).to(dev)
        want = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev).repeat(-(-npages // len(uniq)))[:total]
        c_off, c_len = i64(starts[::PER_CHUNK]), i64(ends[PER_CHUNK - 1::PER_CHUNK] - starts[::PER_CHUNK])
        o_off, o_cap = i64(np.arange(nch) * PER_CHUNK * size), i64(np.full(nch, PER_CHUNK * size))
        b_off, b_len = i64(starts + np.array([heads[k] for k in order])), i64([len(bodies[k]) for k in order])
        p_off, p_cap = i64(np.arange(npages) * size), i64(np.full(npages, size))
        back = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        res, p_res = torch.empty(nch, dtype=torch.int64, device=dev), torch.empty(npages, dtype=torch.int64, device=dev)
    label = "%d chunks of %d x %d B pages" % (nch, PER_CHUNK, size)
    ev = timed(lambda: PLAIN_DECODE[codec](comp, b_off, b_len, back, p_off, p_cap, result=p_res, **kw), side)
    assert int(p_res.min()) == size and torch.equal(back[:total], want)
    base = statistics.median(ev)
    say(codec=codec, page=size, what="yardstick: %d page bodies pre-split with known lengths" % npages, GBps=round(total / base / 1e6, 2), **stats(ev))
    back.zero_()
    ev = timed(lambda: batch.parquet_decompress_chunks_device(comp, c_off, c_len, back, o_off, o_cap, codec, result=res, **kw), side)
    assert int(res.min()) == PER_CHUNK * size and torch.equal(back[:total], want)
    t = statistics.median(ev)
    say(codec=codec, page=size, what="decode: " + label, GBps=round(total / t / 1e6, 2), over_presplit=round(t / base, 3), **stats(ev))
    ev = timed(lambda: batch.parquet_decompress_chunks_device(comp, c_off, c_len, back, o_off, o_cap, codec, verify_crc=True, result=res, **kw), side)
    assert int(res.min()) == PER_CHUNK * size
    tv = statistics.median(ev)
    say(codec=codec, page=size, what="decode with CRC verification", GBps=round(total / tv / 1e6, 2), over_presplit=round(tv / base, 3),
        crc_pass_GBps_of_file_bytes=round(len(blob) / max(tv - t, 1e-6) / 1e6, 2), **stats(ev))
    ev = timed(lambda: batch.parquet_chunk_sizes_device(comp, c_off, c_len, codec, result=res, **kw), side)
    assert int(res.min()) == PER_CHUNK * size
    say(codec=codec, page=size, what="size query alone", share_of_decode=round(statistics.median(ev) / t, 3), **stats(ev))


def main():
    side = torch.cuda.Stream()
    for codec in [c for c in M.REAL if c in sys.argv] or list(M.REAL):
        for size in (65536, 1 << 20):
            try:
                one(codec, size, side)
            except AssertionError as ex:        # a figure that does not hold is reported, the others still measured
                say(codec=codec, page=size, what="FAILED", error=repr(ex)[:300])


if __name__ == "__main__":
    main()
