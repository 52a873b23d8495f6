"""Rates of the frame batches (cj_frame_batch_host / _device) against a Python loop of single calls and the raw-block batch on the same
payload.  Usage: python tests/perf/frame_batch_rates.py [--quick].  One JSON line per case: GB/s of uncompressed bytes."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle  # noqa: E402
import cramjam_amd as cj  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return min(t)


def device_rate(fn, inputs, caps, reps):
    eng = batch._engine(0)
    ln = np.array([len(b) for b in inputs], np.uint64)
    off = np.concatenate([[0], np.cumsum((ln + 15) & ~np.uint64(15))[:-1]]).astype(np.uint64)
    buf = np.zeros(int(off[-1] + ln[-1]) + 64, np.uint8)
    for k, b in enumerate(inputs):
        buf[int(off[k]):int(off[k]) + len(b)] = np.frombuffer(b, np.uint8)
    cap = np.array(caps, np.uint64)
    ooff = np.concatenate([[0], np.cumsum((cap + 15) & ~np.uint64(15))[:-1]]).astype(np.uint64)
    d_in, d_out = eng.alloc(buf.nbytes), eng.alloc(int(ooff[-1] + cap[-1]) + 64)
    rows = [eng.alloc(8 * len(inputs)) for _ in range(5)]
    try:
        eng.h2d(d_in, buf)
        for p, a in zip(rows, (off, ln, ooff, cap)):
            eng.h2d(p, a)
        fmt, op = fn

        def go():
            eng.frame_batch_device(fmt, op, 0, len(inputs), d_in, rows[0], rows[1], d_out, rows[2], rows[3], rows[4])
            eng.sync()
        return best(go, reps)
    finally:
        for p in [d_in, d_out] + rows:
            eng.free(p)


def main():
    quick = "--quick" in sys.argv
    reps = 2 if quick else 5
    cases = [("10000x64KiB", 1000 if quick else 10000, 65536), ("1000x1MiB", 100 if quick else 1000, 1 << 20)]
    uniq = [oracle.synth_v1(1 << 20, i) for i in range(8)]
    for name, n, size in cases:
        raws = [uniq[i % 8][:size] for i in range(n)]
        total = n * size
        for fmt_name, fmt, comp, dec, hc, hd, blk_c, blk_d in (
                ("lz4", N.FORMAT_LZ4_FRAME, cj.lz4.compress, cj.lz4.decompress, batch.lz4_compress_frames, batch.lz4_decompress_frames,
                 lambda p: batch.lz4_compress_blocks(p, store_size=False), lambda b, ls: batch.lz4_decompress_blocks(b, ls)),
                ("snappy", N.FORMAT_SNAPPY_FRAMED, cj.snappy.compress, cj.snappy.decompress, batch.snappy_compress_framed_many,
                 batch.snappy_decompress_framed_many, batch.snappy_compress_raw_many, lambda b, ls: batch.snappy_decompress_raw_many(b))):
            frames = [bytes(f) for f in hc(raws)[1]]
            pieces = [r[k:k + 65536] for r in raws for k in range(0, len(r), 65536)]
            blocks = [bytes(b) for b in blk_c(pieces)[1]]
            L = N.lib()
            caps_c = [(L.cj_lz4_frame_compress_bound if fmt == 0 else L.cj_snappy_frame_max_compress_len)(size)] * n
            rec = {"case": name, "format": fmt_name, "GB": total / 1e9}
            rec["host_decompress"] = total / best(lambda: hd(frames, output_lens=[size] * n), reps) / 1e9
            rec["host_compress"] = total / best(lambda: hc(raws), reps) / 1e9
            rec["device_decompress"] = total / device_rate((fmt, N.OP_DECOMPRESS), frames, [size] * n, reps) / 1e9
            rec["device_compress"] = total / device_rate((fmt, N.OP_COMPRESS), raws, caps_c, reps) / 1e9
            rec["raw_block_host_decompress"] = total / best(lambda: blk_d(blocks, [len(p) for p in pieces]), reps) / 1e9
            m = min(n, 500)
            rec["single_call_loop_decompress"] = m * size / best(lambda: [dec(f) for f in frames[:m]], 1) / 1e9
            rec["single_call_loop_compress"] = m * size / best(lambda: [comp(r) for r in raws[:m]], 1) / 1e9
            print(json.dumps(rec), flush=True)
    big = b"".join(uniq) * (1 if quick else 8)
    f = bytes(cj.lz4.compress(big))
    t_b = best(lambda: batch.lz4_decompress_frames([f], output_lens=[len(big)]), reps)
    t_s = best(lambda: cj.lz4.decompress(f), reps)
    print(json.dumps({"case": "one %d MiB LZ4 frame" % (len(big) >> 20), "batch_GBps": len(big) / t_b / 1e9, "single_call_GBps": len(big) / t_s / 1e9,
                      "batch_ms": t_b * 1e3, "single_ms": t_s * 1e3}), flush=True)


if __name__ == "__main__":
    main()
