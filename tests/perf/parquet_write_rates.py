"""Rates of the Parquet writer on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS runs with
min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/parquet_write_rates.py [--quick] [snappy gzip zstd lz4_raw]      (--quick: one pass at a sixteenth of the size)
Per codec, the workload of parquet_rates.py: the benchmark corpus (tests/golden/corpus) cut into pages of 64 KiB, 16 pages a chunk, V1
pages, repeated to about TOTAL bytes (256 chunks):
  the encode with a CRC on every page; the encode without CRCs; and the plain encoder batch of the same page bodies (the container's
  yardstick: what a caller who then wrote the headers and CRCs on the host would run).  GB/s of decoded (input) bytes."""
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
import parquet_write_model as W  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9
TOTAL = (256 << 20) // (16 if QUICK else 1)
PER_CHUNK, SIZE = 16, 65536
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


PLAIN_ENCODE = {
    "gzip": lambda *a, **kw: batch.deflate_compress_many_device(*a, wrapper="gzip", **kw),
    "snappy": batch.snappy_compress_raw_many_device,
    "lz4_raw": lambda *a, **kw: batch.lz4_compress_blocks_device(*a, store_size=False, **kw),
    "zstd": batch.zstd_compress_many_device,
}


def one(codec, side):
    kw = dict(stream=side.cuda_stream, sync=False)
    data = b"".join(bz2.decompress(open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*.bz2"))))
    uniq = len(data) // SIZE
    npages = max(PER_CHUNK, TOTAL // SIZE // PER_CHUNK * PER_CHUNK)
    nch, total = npages // PER_CHUNK, npages * SIZE
    slot = (W.slot_bound(codec, SIZE) + 15) // 16 * 16
    cap = (batch.parquet_compress_bound(codec, PER_CHUNK * SIZE, PER_CHUNK) + 15) // 16 * 16
    rows = np.array(W.table_of([dict(type=0, usize=SIZE, num_values=SIZE // 8, def_enc=3, rep_enc=3)] * PER_CHUNK), np.int64)
    with torch.cuda.stream(side):
        plain = torch.from_numpy(np.frombuffer(data[:uniq * SIZE], np.uint8).copy()).to(dev).repeat(-(-npages // uniq))[:total].contiguous()
        t_rows, t_nocrc = i64(rows.reshape(-1)), i64(np.array(W.with_crc(rows.tolist(), False), np.int64).reshape(-1))
        r_off, r_cnt = i64(np.zeros(nch)), i64(np.full(nch, PER_CHUNK))
        c_off, c_len = i64(np.arange(nch) * PER_CHUNK * SIZE), i64(np.full(nch, PER_CHUNK * SIZE))
        o_off, o_cap = i64(np.arange(nch) * cap), i64(np.full(nch, cap))
        p_off, p_len = i64(np.arange(npages) * SIZE), i64(np.full(npages, SIZE))
        s_off, s_cap = i64(np.arange(npages) * slot), i64(np.full(npages, slot))
        out = torch.zeros(max(nch * cap, npages * slot) + 64, dtype=torch.uint8, device=dev)
        back = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        res, p_res = torch.empty(nch, dtype=torch.int64, device=dev), torch.empty(npages, dtype=torch.int64, device=dev)
    label = "%d chunks of %d x %d B pages" % (nch, PER_CHUNK, SIZE)
    ev = timed(lambda: PLAIN_ENCODE[codec](plain, p_off, p_len, out, s_off, s_cap, result=p_res, **kw), side)
    assert int(p_res.min()) > 0
    base, packed = statistics.median(ev), int(p_res.sum())
    say(codec=codec, what="yardstick: the plain encoder batch of %d page bodies" % npages, GBps=round(total / base / 1e6, 2), ratio=round(total / packed, 3), **stats(ev))
    for name, tab in (("encode, a CRC on every page: " + label, t_rows), ("encode without CRCs", t_nocrc)):
        ev = timed(lambda: batch.parquet_compress_chunks_device(plain, c_off, c_len, tab, r_off, r_cnt, out, o_off, o_cap, codec, result=res, **kw), side)
        assert int(res.min()) > 0
        t = statistics.median(ev)
        say(codec=codec, what=name, GBps=round(total / t / 1e6, 2), over_yardstick=round(t / base, 3), ratio=round(total / int(res.sum()), 3), **stats(ev))
    # what was written decodes to the input, CRCs verified
    batch.parquet_decompress_chunks_device(out, o_off, res, back, c_off, c_len, codec, verify_crc=tab is t_rows, result=p_res[:nch], stream=side.cuda_stream, sync=True)
    assert int(p_res[:nch].min()) == PER_CHUNK * SIZE and torch.equal(back[:total], plain)


def main():
    side = torch.cuda.Stream()
    for codec in [c for c in M.REAL if c in sys.argv] or list(M.REAL):
        try:
            one(codec, side)
        except AssertionError as ex:            # a figure that does not hold is reported, the others still measured
            say(codec=codec, what="FAILED", error=repr(ex)[:300])


if __name__ == "__main__":
    main()
