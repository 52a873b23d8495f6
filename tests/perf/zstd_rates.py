"""Rates of the Zstandard batch decoder (cj_zstd_batch_device) on device-resident batches, with libzstd's
ZSTD_decompress on 16 threads over the same streams as the CPU baseline.  Level-3 streams of 64 KiB text-like chunks and of 4 KiB
records, with and without content checksum; `unique` different streams referenced round-robin by the batch's offsets, every chunk
with an output slot of its own.  Prints one JSON line per configuration.
usage: python tests/perf/zstd_rates.py [--chunks64k 100000] [--records4k 400000] [--unique 256] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_cases as Z  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def corpus_chunk(words, n, seed):
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += b" ".join(rnd.choice(words) for _ in range(48)) + b" %d\n" % rnd.randrange(10 ** 6)
    return bytes(out[:n])


def cpu_rate(streams, size, total_chunks):
    L = Z.libzstd()
    per = max(1, min(total_chunks, 20000) // 16)

    def work(t):
        out = C.create_string_buffer(size)
        for k in range(per):
            s = streams[(t * per + k) % len(streams)]
            assert L.ZSTD_decompress(out, size, s, len(s)) == size
    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        list(ex.map(work, range(16)))
        dt = time.perf_counter() - t0
    return 16 * per * size / dt / 1e9


def gpu_rate(streams, size, n, reps):
    off, run = [], 0
    for s in streams:
        off.append(run)
        run += (len(s) + 15) // 16 * 16 + 16
    blob = np.zeros(run + 64, np.uint8)
    for o, s in zip(off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, np.uint8)
    idx = np.arange(n) % len(streams)
    t_in = torch.from_numpy(blob).cuda()
    t_off = torch.from_numpy(np.array(off, np.int64)[idx]).cuda()
    t_len = torch.from_numpy(np.array([len(s) for s in streams], np.int64)[idx]).cuda()
    t_cap = torch.full((n,), size, dtype=torch.int64, device="cuda")
    t_ooff = torch.arange(n, dtype=torch.int64, device="cuda") * size
    t_out = torch.empty(n * size + 64, dtype=torch.uint8, device="cuda")
    res = torch.empty(n, dtype=torch.int64, device="cuda")
    times = []
    for _ in range(reps + 1):                                  # the first run also grows the engine's literal slots
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.zstd_decompress_many_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, result=res, sync=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        times.append(dt)
    best = min(times[1:])
    assert bool((res == size).all())
    first = t_out[:size].cpu().numpy().tobytes()
    assert Z.zstd_verdict(streams[0], size)[1] == first
    return n * size / best / 1e9, best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks64k", type=int, default=100000)
    ap.add_argument("--records4k", type=int, default=400000)
    ap.add_argument("--unique", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    words = open(os.path.join(os.path.dirname(HERE), "golden", "plaintext.txt"), "rb").read().split()
    for name, size, n in (("64KiB corpus chunks", 65536, a.chunks64k), ("4KiB records", 4096, a.records4k)):
        payloads = [corpus_chunk(words, size, 1000 * size + k) for k in range(a.unique)]
        for checksum in (0, 1):
            streams = [Z.zstd_compress(p, level=3, checksum=checksum) for p in payloads]
            ratio = sum(len(p) for p in payloads) / sum(len(s) for s in streams)
            gbs, ms = gpu_rate(streams, size, n, a.reps)
            cpu = cpu_rate(streams, size, n)
            print(json.dumps(dict(workload="zstd level-3 decode, %d x %s, device-resident" % (n, name), checksum=bool(checksum), ratio=round(ratio, 3),
                                  gpu_GBps=round(gbs, 2), gpu_ms=round(ms, 2), cpu16_GBps=round(cpu, 2), libzstd=Z.libzstd().ZSTD_versionString().decode())), flush=True)


if __name__ == "__main__":
    main()
