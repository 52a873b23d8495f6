"""Rates of the ORC stream batches on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS runs
with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/orc_rates.py [--quick] [zlib snappy lz4 zstd]      (--quick: one pass at a sixteenth of the size)
Per codec, over the benchmark corpus (tests/golden/corpus) cut into 64 KiB chunks, repeated to CHUNKS chunks, as streams of 16 chunks
at block_size 65 536 — written by this library's ORC encoder, so some chunks are original:
  the ORC decode; the size query alone; the plain batch of the same compressed chunks pre-split with known lengths (the container's
  yardstick: what a caller who had walked the headers and knew every length would run); the ORC encode against the plain encoder
  batch of the same pieces."""
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
import orc_model as M  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9
BS = 65536
PER_STREAM = 16
CHUNKS = 16384 // (16 if QUICK else 1)
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


def corpus_chunks():
    data = b"".join(bz2.decompress(open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "corpus", "*.bz2"))))
    return [data[i:i + BS] for i in range(0, len(data) - BS + 1, BS)]


PLAIN_DECODE = {
    "zlib": lambda *a, **kw: batch.deflate_decompress_many_device(*a, wrapper="raw", **kw),
    "snappy": batch.snappy_decompress_raw_many_device,
    "lz4": lambda *a, **kw: batch.lz4_decompress_blocks_device(*a, store_size=False, **kw),
    "zstd": batch.zstd_decompress_many_device,
}
PLAIN_ENCODE = {
    "zlib": (lambda *a, **kw: batch.deflate_compress_many_device(*a, wrapper="raw", **kw), lambda L: L.cj_deflate_compress_bound(BS, N.DEFLATE_RAW)),
    "snappy": (batch.snappy_compress_raw_many_device, lambda L: L.cj_snappy_raw_max_compress_len(BS)),
    "lz4": (lambda *a, **kw: batch.lz4_compress_blocks_device(*a, store_size=False, **kw), lambda L: L.cj_lz4_block_compress_bound(BS, 0)),
    "zstd": (batch.zstd_compress_many_device, lambda L: L.cj_zstd_compress_bound(BS, 0)),
}


def one_codec(codec, raw, side):
    s = side.cuda_stream
    kw = dict(stream=s, sync=False)
    ns, total = CHUNKS // PER_STREAM, CHUNKS * BS
    span = PER_STREAM * BS
    bound = batch.orc_compress_bound(span, BS)
    with torch.cuda.stream(side):
        b_off, b_len = i64(np.arange(ns) * span), i64(np.full(ns, span))
        s_off, s_cap = i64(np.arange(ns) * bound), i64(np.full(ns, bound))
        comp = torch.empty(ns * bound + 64, dtype=torch.uint8, device=dev)
        s_len = torch.empty(ns, dtype=torch.int64, device=dev)
        back = torch.empty(total + 64, dtype=torch.uint8, device=dev)
        res = torch.empty(ns, dtype=torch.int64, device=dev)
    # ---- encode
    ev = timed(lambda: batch.orc_compress_streams_device(raw, b_off, b_len, comp, s_off, s_cap, codec, BS, result=s_len, **kw), side)
    lens = s_len.cpu().numpy()
    assert lens.min() > 0
    orc_enc = statistics.median(ev)
    say(codec=codec, what="encode: %d buffers of %d x %d B into ORC streams" % (ns, PER_STREAM, BS), GBps=round(total / orc_enc / 1e6, 2), ratio=round(total / int(lens.sum()), 3), **stats(ev))
    enc, bound_of = PLAIN_ENCODE[codec]
    stride = (bound_of(N.lib()) + 15) // 16 * 16
    with torch.cuda.stream(side):
        p_off, p_len = i64(np.arange(CHUNKS) * BS), i64(np.full(CHUNKS, BS))
        c_off, c_cap = i64(np.arange(CHUNKS) * stride), i64(np.full(CHUNKS, stride))
        pieces = torch.empty(CHUNKS * stride + 64, dtype=torch.uint8, device=dev)
        c_res = torch.empty(CHUNKS, dtype=torch.int64, device=dev)
    ev = timed(lambda: enc(raw, p_off, p_len, pieces, c_off, c_cap, result=c_res, **kw), side)
    assert int(c_res.min()) > 0
    t = statistics.median(ev)
    say(codec=codec, what="encode yardstick: the same %d pieces as a plain batch" % CHUNKS, GBps=round(total / t / 1e6, 2), orc_over_it=round(orc_enc / t, 3), **stats(ev))
    del pieces
    # ---- the chunk rows, from a walk on the host (the yardstick gets the compressed chunks pre-split, with their lengths)
    host = comp.cpu().numpy()
    m_off, m_len, d_off, norig = [], [], [], 0
    for i in range(ns):
        base = i * bound
        code, chunks = M.walk(host[base:base + int(lens[i])].tobytes())
        assert code == 0 and len(chunks) == PER_STREAM
        for k, (off, n, orig) in enumerate(chunks):
            if orig:
                norig += 1
            else:
                m_off.append(base + off); m_len.append(n); d_off.append((i * PER_STREAM + k) * BS)
    nc = len(m_off)
    with torch.cuda.stream(side):
        t_moff, t_mlen, t_doff, t_dcap = i64(m_off), i64(m_len), i64(d_off), i64(np.full(nc, BS))
        m_res = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)[:nc]
    # ---- decode
    base_ms = None
    if nc:
        ev = timed(lambda: PLAIN_DECODE[codec](comp, t_moff, t_mlen, back, t_doff, t_dcap, result=m_res, **kw), side)
        assert int(m_res.min()) == BS
        base_ms = statistics.median(ev)
        say(codec=codec, what="decode yardstick: %d compressed chunks pre-split with known lengths (%d more are original)" % (nc, norig),
            GBps=round(nc * BS / base_ms / 1e6, 2), **stats(ev))
    back.zero_()
    ev = timed(lambda: batch.orc_decompress_streams_device(comp, s_off, s_len, back, b_off, b_len, codec, BS, result=res, **kw), side)
    assert int(res.min()) == span and torch.equal(back[:total], raw[:total])
    t = statistics.median(ev)
    say(codec=codec, what="decode: %d ORC streams of %d chunks" % (ns, PER_STREAM), GBps=round(total / t / 1e6, 2),
        over_presplit=round(t / base_ms, 3) if base_ms else None, **stats(ev))
    ev = timed(lambda: batch.orc_stream_sizes_device(comp, s_off, s_len, codec, BS, result=res, **kw), side)
    assert int(res.min()) == span
    ts = statistics.median(ev)
    say(codec=codec, what="size query alone", share_of_decode=round(ts / t, 3), **stats(ev))


def main():
    side = torch.cuda.Stream()
    uniq = corpus_chunks()
    reps = -(-CHUNKS // len(uniq))
    with torch.cuda.stream(side):
        raw = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev).repeat(reps)[:CHUNKS * BS]
        raw = torch.cat([raw, torch.zeros(64, dtype=torch.uint8, device=dev)])
    side.synchronize()
    for codec in [c for c in M.KINDS if c in sys.argv] or list(M.KINDS):
        one_codec(codec, raw, side)


if __name__ == "__main__":
    main()
