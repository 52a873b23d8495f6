"""Rates of the decoded-size queries (cj_batch_sizes_device, cj_frame_batch_sizes_device) on one MI355X — DESIGN.md 5.9.
Device-resident batches built like bench.py's (build_batch: synth-v1 or corpus chunks compressed by liblz4, replicated to distinct
addresses); a figure = the median of RUNS runs, a run = K submissions between two events on a side stream after a warm-up, with
the run-to-run spread (min .. max) next to it.
    python tests/perf/batch_sizes_rates.py [--quick] [--only NAME]
--only lz4-64k runs the 100 000-chunk batch alone, query and decode alternating: under `rocprofv3 --kernel-trace --stats` that gives
lz4_size_lanes_kernel next to lz4_parse_kernel on the same chunks in one process."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import oracle  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

RUNS, K = 7, 5
DEV = torch.device("cuda:0")


def timed(side, submit):
    """median / min / max over RUNS of the time per submission, ms"""
    ms = []
    with torch.cuda.stream(side):
        for _ in range(2):
            submit()
        side.synchronize()
        for _ in range(RUNS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(side)
            for _ in range(K):
                submit()
            t1.record(side)
            t1.synchronize()
            ms.append(t0.elapsed_time(t1) / K)
    return statistics.median(ms), min(ms), max(ms)


def show(name, what, t, nbytes_in, nbytes_out, n):
    print("%-14s %-22s %8.3f ms (%.3f .. %.3f)  %8.1f GB/s of input  %9.1f GB/s of decoded size  %7.1f M chunks/s"
          % (name, what, t[0], t[1], t[2], nbytes_in / t[0] / 1e6, nbytes_out / t[0] / 1e6, n / t[0] / 1e3), flush=True)


def lz4_batch(name, S, NCH, data, eng, side, decode=True):
    L = N.lib()
    U = min(2048, NCH)
    if data == "corpus64k":
        U = min(U, len(bench.corpus_chunks(S)[0]))
    b = bench.build_batch(N, L, eng, DEV, N.CODEC_LZ4_BLOCK, True, S, U, NCH, 0, "auto", torch, np, data)
    mp = b.meta.data_ptr()
    t_res = torch.empty(NCH, dtype=torch.int64, device=DEV)
    s = side.cuda_stream
    torch.cuda.synchronize()

    def q():
        N.check(L.cj_batch_sizes_device(eng.h, N.CODEC_LZ4_BLOCK, 0, NCH, b.cin.data_ptr(), mp, mp + 8 * NCH, t_res.data_ptr(), s))
    tq = timed(side, q)
    assert (t_res.cpu().numpy() == S).all()
    show(name, "size query (%s)" % (b.comp_name or "").split(" ")[0], tq, b.bytes_in, b.bytes_out, NCH)
    if decode:
        def d():
            eng.batch_device(N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, 0, NCH, b.cin.data_ptr(), mp, mp + 8 * NCH, b.out.data_ptr(), mp + 16 * NCH, mp + 24 * NCH, mp + 32 * NCH, s)
        td = timed(side, d)
        show(name, "decode", td, b.bytes_in, b.bytes_out, NCH)
        print("%-14s query / (query + decode) = %.3f" % (name, tq[0] / (tq[0] + td[0])), flush=True)
    del b


def header_and_frames(eng, side, n=10000):
    L = N.lib()
    raw = oracle.synth_v1(65536, 1) + oracle.synth_v1(65536, 2) + oracle.synth_v1(65536, 3) + oracle.synth_v1(65536, 4)
    items = {"snappy-raw": (oracle.snappy_compress(raw[:65536])[1], L.cj_batch_sizes_device, N.CODEC_SNAPPY_RAW, 0),
             "lz4-prefixed": ((65536).to_bytes(4, "little") + oracle.lz4_compress_raw(raw[:65536])[1], L.cj_batch_sizes_device, N.CODEC_LZ4_BLOCK, 1),
             "lz4-frames": (oracle.lz4_frame_compress(raw, 4, 0)[1], L.cj_frame_batch_sizes_device, N.FORMAT_LZ4_FRAME, 0),
             "snappy-framed": (oracle.snappy_frame_compress(raw)[1], L.cj_frame_batch_sizes_device, N.FORMAT_SNAPPY_FRAMED, 0)}
    for name, (blob, fn, what, flags) in items.items():
        pitch = (len(blob) + 15) & ~15
        one = np.zeros(pitch, np.uint8)
        one[:len(blob)] = np.frombuffer(blob, np.uint8)
        t_in = torch.from_numpy(one).to(DEV).repeat(n)
        meta = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.uint64) * np.uint64(pitch), np.full(n, len(blob), np.uint64)]).view(np.int64)).to(DEV)
        t_res = torch.empty(n, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        t = timed(side, lambda: N.check(fn(eng.h, what, flags, n, t_in.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8 * n, t_res.data_ptr(), side.cuda_stream)))
        r = t_res.cpu().numpy()
        assert (r == r[0]).all() and r[0] > 0
        show(name, "query (result %d)" % r[0], t, n * len(blob), n * int(r[0]), n)


def host_decode_with_and_without_lengths(n=16384):
    raws = [oracle.synth_v1(65536, i) for i in range(256)]
    comp = [oracle.lz4_compress_raw(r)[1] for r in raws]
    blocks = [comp[i % 256] for i in range(n)]
    lens = [65536] * n
    out = bytearray(n * 65536)
    for what, call in (("with output_lens", lambda: batch.lz4_decompress_blocks(blocks, lens, out=out)),
                       ("output_lens=None", lambda: batch.lz4_decompress_blocks(blocks, out=out)),
                       ("lz4_block_sizes", lambda: batch.lz4_block_sizes(blocks))):
        call()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = call()
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        print("host 16384x64K  %-18s %8.1f ms (%.1f .. %.1f)  %6.2f GB/s of output" % (what, t * 1e3, min(ts) * 1e3, max(ts) * 1e3, n * 65536 / t / 1e9), flush=True)


def main():
    global RUNS
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    eng = N.Engine(0)
    side = torch.cuda.Stream()
    print("device: %s; %d runs of %d submissions per figure: median (min .. max)" % (torch.cuda.get_device_name(0), RUNS, K), flush=True)
    if args.only == "lz4-64k":
        lz4_batch("lz4-64k", 65536, 100000, "synth-v1", eng, side)
        return
    scale = 10 if args.quick else 1
    lz4_batch("lz4-64k", 65536, 100000 // scale, "synth-v1", eng, side)
    lz4_batch("lz4-16k", 16384, 400000 // scale, "synth-v1", eng, side)
    lz4_batch("corpus-64k", 65536, 100000 // scale, "corpus64k", eng, side)
    lz4_batch("lz4-256k", 262144, 8192 // scale, "synth-v1", eng, side, decode=False)
    header_and_frames(eng, side, 10000 // scale)
    host_decode_with_and_without_lengths(16384 // scale)
    eng.close()


if __name__ == "__main__":
    main()
