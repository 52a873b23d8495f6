"""Rates of the Blosc chunk path on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS runs
with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/blosc_rates.py [--quick]      (--quick: one pass of every batch, for a kernel trace)"""
import ctypes as C
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
import make_golden_blosc as G  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9


def say(**kw):
    print(json.dumps(kw), flush=True)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def timed(fn, side):
    """HIP events on the side stream around fn; also the wall clock of the call with its wait"""
    ev, wall = [], []
    for k in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        side.synchronize()
        t = time.perf_counter()
        a.record(side)
        fn()
        b.record(side)
        side.synchronize()
        if k or QUICK:
            ev.append(a.elapsed_time(b)); wall.append((time.perf_counter() - t) * 1e3)
    return ev, wall


def filters(eng):
    total, blk = (1 << 30) if QUICK else (4 << 30), 262144
    n = total // blk
    src, dst = eng.alloc(total), eng.alloc(total)
    N.check(N.lib().cj_memset_dev(eng.h, src, 0x5B, total))
    ms = C.c_double(0)

    def run(forward, filt, ts):
        out = []
        for k in range(RUNS + 1):
            N.check(N.lib().cj_debug_blosc_filter(eng.h, forward, filt, ts, src, dst, blk, blk, n, C.byref(ms)))
            if k or QUICK:
                out.append(ms.value)
        return out
    copy = run(0, 3, 1)
    say(what="filter yardstick: device-to-device copy", bytes=total, GBps_read_plus_write=round(2 * total / statistics.median(copy) / 1e6, 1), **stats(copy))
    for ts in (2, 4, 8, 16, 7):
        for filt, fname in ((1, "shuffle"), (2, "bitshuffle")):
            for forward in (1, 0):
                t = run(forward, filt, ts)
                say(what="%s%s" % ("" if forward else "un", fname), typesize=ts, block=blk, bytes=total,
                    GBps_read_plus_write=round(2 * total / statistics.median(t) / 1e6, 1), times_the_copy=round(statistics.median(t) / statistics.median(copy), 2), **stats(t))
    eng.free(src); eng.free(dst)


def stream_rows(chunks_host, coff, n):
    """the LZ4 streams of the chunks as a plain block batch: offsets into the same device blob"""
    off, ln, cap = [], [], []
    for i in range(n):
        c = chunks_host[i]
        for s in M.parse(c)[1]:
            if not s[5]:
                off.append(int(coff[i]) + s[0]); ln.append(s[1]); cap.append(s[3])
    return off, ln, cap


def device_batches(side, label, raw, n, S, comp=None, coff=None, clen=None):
    dev = raw.device
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
    off, ln = i64(np.arange(n) * S), i64(np.full(n, S))
    res = torch.empty(n, dtype=torch.int64, device=dev)
    if comp is None:                                               # this library's compressor
        stride = S + 32
        coff_h = np.arange(n) * stride
        comp = torch.empty(n * stride + 64, dtype=torch.uint8, device=dev)
        ev, wall = timed(lambda: batch.blosc_compress_chunks_device(raw, off, ln, comp, i64(coff_h), i64(np.full(n, stride)), 4, filter=1, result=res,
                                                                   stream=side.cuda_stream), side)
        clen_h = res.cpu().numpy()
        say(what=label + ": blosc compress, whole call (events)", chunks=n, chunk_bytes=S, GBps=round(n * S / statistics.median(ev) / 1e6, 1),
            ratio=round(n * S / float(clen_h.sum()), 3), wall_median_ms=round(statistics.median(wall), 3), **stats(ev))
    else:
        coff_h, clen_h = coff, clen
    back = torch.empty(n * S, dtype=torch.uint8, device=dev)
    d_coff, d_clen = i64(coff_h), i64(clen_h)
    ev, wall = timed(lambda: batch.blosc_decompress_chunks_device(comp, d_coff, d_clen, back, off, ln, result=res, stream=side.cuda_stream), side)
    assert torch.equal(back, raw) and int(res.min()) == S
    blosc_ms = statistics.median(ev)
    say(what=label + ": blosc decompress, whole call (events)", chunks=n, chunk_bytes=S, GBps=round(n * S / blosc_ms / 1e6, 1),
        wall_median_ms=round(statistics.median(wall), 3), **stats(ev))
    # yardstick: the same LZ4 streams as a plain block batch (the engine's kernels are the parent commit's: this change touches none)
    host = comp.cpu().numpy()
    chunks = [host[int(coff_h[i]):int(coff_h[i]) + int(clen_h[i])].tobytes() for i in range(n)]
    soff, sln, scap = stream_rows(chunks, coff_h, n)
    if soff:
        ooff = np.concatenate([[0], np.cumsum((np.asarray(scap) + 15) // 16 * 16)[:-1]])
        plain = torch.empty(int(ooff[-1] + scap[-1]) + 64, dtype=torch.uint8, device=dev)
        d = [i64(soff), i64(sln), i64(ooff), i64(scap)]
        r2 = torch.empty(len(soff), dtype=torch.int64, device=dev)
        flags_cap = max(scap)
        ev2, _ = timed(lambda: batch.lz4_decompress_blocks_device(comp, d[0], d[1], plain, d[2], d[3], result=r2, stream=side.cuda_stream), side)
        lz4_ms = statistics.median(ev2)
        say(what=label + ": the same LZ4 streams through lz4_decompress_blocks_device", streams=len(soff), longest_stream=flags_cap,
            GBps=round(sum(scap) / lz4_ms / 1e6, 1), **stats(ev2))
        say(what=label + ": container cost of the decode (blosc call - plain block batch)", ms=round(blosc_ms - lz4_ms, 4))
    return comp, coff_h, clen_h, chunks


def main():
    side = torch.cuda.Stream()
    eng = batch._engine(0)
    filters(eng)
    n, S = (2000 if QUICK else 10000), 262144
    with torch.cuda.stream(side):
        raw = (torch.arange(n * S // 4, dtype=torch.float32, device="cuda") * 0.25).view(torch.uint8)
        comp, coff, clen, chunks = device_batches(side, "10 000 x 256 KiB float32 ramp, this library's chunks (64 KiB streams)", raw, n, S)
    lib = G.load_libblosc()
    say(what="libblosc", loaded=lib is not None)
    if lib is not None:
        # libblosc's own shape: 1 MiB of the same ramp per chunk, lz4 clevel 5, typesize 4: 512 KiB blocks of four 128 KiB streams
        S2, uniq = 1 << 20, 64
        n2 = (n * S) // S2 // uniq * uniq
        host = raw[:uniq * S2].cpu().numpy()
        lb = [G.mint(lib, host[k * S2:(k + 1) * S2].tobytes(), dict(clevel=5, filter=1, typesize=4, cname="lz4", blocksize=0, split=4)) for k in range(uniq)]
        ours = batch.blosc_compress_chunks([host[k * S2:(k + 1) * S2] for k in range(uniq)], 4)[0]
        say(what="ratio on 64 x 1 MiB of the ramp", libblosc_lz4_clevel5=round(uniq * S2 / sum(map(len, lb)), 3), this_library=round(uniq * S2 / sum(ours), 3))
        h, st = M.parse(lb[0])
        say(what="libblosc chunk shape", blocksize=h["blocksize"], streams=len(st), stream_bytes=st[0][3])
        blob, off, ln = [], [], []
        run = 0
        for i in range(n2):
            c = lb[i % uniq]
            off.append(run); ln.append(len(c)); blob.append(np.frombuffer(c, np.uint8)); pad = -len(c) % 16 + 16
            blob.append(np.zeros(pad, np.uint8)); run += len(c) + pad
        with torch.cuda.stream(side):
            raw2 = torch.cat([raw[:uniq * S2]] * (n2 // uniq))
            comp2 = torch.from_numpy(np.concatenate(blob + [np.zeros(64, np.uint8)])).cuda()
            device_batches(side, "%d x 1 MiB, libblosc's chunks (128 KiB streams)" % n2, raw2, n2, S2, comp2, np.asarray(off), np.asarray(ln))
        # CPU baseline: blosc_decompress_ctx with 16 threads on this library's chunks
        out = C.create_string_buffer(S)
        k = min(n, 2000)
        t = time.perf_counter()
        for c in chunks[:k]:
            assert lib.blosc_decompress_ctx(c, out, S, 16) == S
        dt = time.perf_counter() - t
        say(what="CPU baseline: blosc_decompress_ctx, 16 threads, chunk after chunk", chunks=k, GBps=round(k * S / dt / 1e9, 2))
    # host batch end to end, next to the plain block batch of the same payload
    k = min(n, 2000)
    buf = bytearray(k * S)
    ts = []
    for _ in range(RUNS + 1):
        t = time.perf_counter(); res, _o = batch.blosc_decompress_chunks(chunks[:k], out=buf); ts.append((time.perf_counter() - t) * 1e3)
    assert res == [S] * k
    say(what="host batch: blosc_decompress_chunks(out=buf)", chunks=k, GBps=round(k * S / statistics.median(ts[1:] or ts) / 1e6, 2), **stats(ts[1:] or ts))
    streams, caps = [], []
    for c in chunks[:k]:
        for s in M.parse(c)[1]:
            if not s[5]:
                streams.append(c[s[0]:s[0] + s[1]]); caps.append(s[3])
    buf2 = bytearray(sum(caps))
    ts = []
    for _ in range(RUNS + 1):
        t = time.perf_counter(); batch.lz4_decompress_blocks(streams, caps, out=buf2); ts.append((time.perf_counter() - t) * 1e3)
    say(what="host batch: lz4_decompress_blocks(out=buf) of the same streams", streams=len(streams), GBps=round(sum(caps) / statistics.median(ts[1:] or ts) / 1e6, 2), **stats(ts[1:] or ts))


if __name__ == "__main__":
    main()
