"""Rates of the LZ4 dictionary batches on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS
runs with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/dict_rates.py [--quick]      (--quick: one pass of every batch at a tenth of the size, for a kernel trace)
Word-like records of the dictionary's vocabulary (tests/lz4_dict_model.py), 256 distinct ones repeated; 64 KiB dictionary."""
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lz4_dict_model as D  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9
UNIQ = 256


def say(**kw):
    print(json.dumps(kw), flush=True)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def timed(fn, side, runs=None):
    ev = []
    runs = RUNS if runs is None else runs
    for k in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        side.synchronize()
        a.record(side)
        fn()
        b.record(side)
        side.synchronize()
        if k or QUICK:
            ev.append(a.elapsed_time(b))
    return ev


def shape(side, eng, n, S, d_host):
    dev = torch.device("cuda:0")
    L = N.lib()
    i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64), device=dev)
    label = "%d x %d B" % (n, S)
    with torch.cuda.stream(side):
        t_dict = torch.from_numpy(np.frombuffer(d_host, np.uint8).copy()).to(dev)
        uniq = [D.words(S, 31000 + k) for k in range(UNIQ)]
        raw_u = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev)
        raw = raw_u.view(UNIQ, S).repeat(n // UNIQ, 1).reshape(-1)
        off, ln = i64(np.arange(n) * S), i64(np.full(n, S))
        bound = L.cj_lz4_block_compress_bound(S, 0)
        stride = (bound + 15) // 16 * 16
        coff, ccap = i64(np.arange(n) * stride), i64(np.full(n, stride))
        comp_d, comp_p = (torch.empty(n * stride + 64, dtype=torch.uint8, device=dev) for _ in range(2))
        res_d, res_p, res = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
        back = torch.empty(n * S + 64, dtype=torch.uint8, device=dev)
    side.synchronize()
    s = side.cuda_stream
    p = lambda t: t.data_ptr()

    def call_dict(op, i, o, r):
        N.check(L.cj_dict_batch_device(eng.h, 0, op, 0, n, p(i[0]), p(i[1]), p(i[2]), p(o[0]), p(o[1]), p(o[2]), p(r), p(t_dict), t_dict.numel(), s))

    def call_plain(op, flags, i, o, r):
        N.check(L.cj_batch_device(eng.h, 0, op, flags, n, p(i[0]), p(i[1]), p(i[2]), p(o[0]), p(o[1]), p(o[2]), p(r), s))

    # ---- encode ----
    one = timed(lambda: call_dict(N.OP_COMPRESS, (raw, off, ln), (comp_d, coff, ccap), res_d), side, runs=1)
    enc_runs = RUNS if one[-1] < 1500 else 3                          # (a pass of more than 1.5 s: the median of 3)
    ev = timed(lambda: call_dict(N.OP_COMPRESS, (raw, off, ln), (comp_d, coff, ccap), res_d), side, runs=enc_runs)
    enc_d = statistics.median(ev)
    say(what=label + ": compress WITH the dictionary (staging + linked encoder)", GBps=round(n * S / enc_d / 1e6, 1), **stats(ev))
    ev = timed(lambda: call_plain(N.OP_COMPRESS, 0, (raw, off, ln), (comp_p, coff, ccap), res_p), side)
    enc_p = statistics.median(ev)
    say(what=label + ": compress without (lz4_compress_blocks_device's call)", GBps=round(n * S / enc_p / 1e6, 1), times_slower_with=round(enc_d / enc_p, 2), **stats(ev))
    assert int(res_d.min()) > 0 and int(res_p.min()) > 0
    say(what=label + ": compressed bytes", with_dictionary=int(res_d.sum()), without=int(res_p.sum()), ratio_with=round(n * S / int(res_d.sum()), 3),
        ratio_without=round(n * S / int(res_p.sum()), 3))
    # ---- decode ----
    ev = timed(lambda: call_dict(N.OP_DECOMPRESS, (comp_d, coff, res_d), (back, off, ln), res), side)
    dec_d = statistics.median(ev)
    assert int(res.min()) == S and torch.equal(back[:n * S], raw)
    say(what=label + ": decompress WITH the dictionary (one wavefront per chunk)", GBps=round(n * S / dec_d / 1e6, 1), **stats(ev))
    back.zero_()
    ev = timed(lambda: call_plain(N.OP_DECOMPRESS, N.FLAG_FORCE_WAVE_PER_CHUNK, (comp_p, coff, res_p), (back, off, ln), res), side)
    dec_w = statistics.median(ev)
    assert int(res.min()) == S and torch.equal(back[:n * S], raw)
    say(what=label + ": yardstick 1, the same records without a dictionary, CJ_FLAG_FORCE_WAVE_PER_CHUNK (the same kernel shape)", GBps=round(n * S / dec_w / 1e6, 1),
        dictionary_decode_over_it=round(dec_d / dec_w, 3), **stats(ev))
    ev = timed(lambda: call_plain(N.OP_DECOMPRESS, N.FLAG_CHUNKS_LE_16K if S <= 16384 else 0, (comp_p, coff, res_p), (back, off, ln), res), side)
    dec_p = statistics.median(ev)
    say(what=label + ": yardstick 2, the same records without a dictionary, the default path (workgroup decoder)", GBps=round(n * S / dec_p / 1e6, 1),
        dictionary_decode_over_it=round(dec_d / dec_p, 3), **stats(ev))
    ev = timed(lambda: N.check(L.cj_dict_batch_sizes_device(eng.h, 0, 0, n, p(comp_d), p(coff), p(res_d), p(res), t_dict.numel(), s)), side)
    assert int(res.min()) == S
    say(what=label + ": size query with the dictionary (one wavefront per chunk)", GBps_of_output=round(n * S / statistics.median(ev) / 1e6, 1), **stats(ev))
    # ---- context: a host batch, and liblz4 on 16 threads ----
    k = min(n, 20000)
    host = comp_d[:k * stride].cpu().numpy()
    lens = res_d[:k].cpu().numpy()
    chunks = [host[i * stride:i * stride + int(lens[i])].tobytes() for i in range(k)]
    buf = bytearray(k * S)
    ts = []
    for _ in range(RUNS + 1):
        t = time.perf_counter(); r, _o = batch.lz4_decompress_blocks(chunks, [S] * k, out=buf, dictionary=d_host); ts.append((time.perf_counter() - t) * 1e3)
    assert list(r) == [S] * k
    say(what=label + ": host batch, lz4_decompress_blocks(out=buf, dictionary=d)", chunks=k, GBps=round(k * S / statistics.median(ts[1:] or ts) / 1e6, 2), **stats(ts[1:] or ts))
    lz = D.liblz4()
    if lz is not None:
        dbuf = C.create_string_buffer(bytes(d_host), len(d_host))
        outs = [C.create_string_buffer(S) for _ in range(16)]

        def work(t):
            for i in range(t, k, 16):
                assert lz.LZ4_decompress_safe_usingDict(chunks[i], outs[t], len(chunks[i]), S, dbuf, len(d_host)) == S
        ts = []
        with ThreadPoolExecutor(16) as ex:
            for _ in range(RUNS + 1):
                t = time.perf_counter(); list(ex.map(work, range(16))); ts.append((time.perf_counter() - t) * 1e3)
        say(what=label + ": CPU context, LZ4_decompress_safe_usingDict on 16 threads", chunks=k, GBps=round(k * S / statistics.median(ts[1:] or ts) / 1e6, 2), **stats(ts[1:] or ts))


def main():
    side = torch.cuda.Stream()
    eng = batch._engine(0)
    d = D.dictionary(65536)
    scale = 10 if QUICK else 1
    for n, S in ((200000 // scale, 4096), (400000 // scale, 16384)):
        shape(side, eng, n // UNIQ * UNIQ, S, d)


if __name__ == "__main__":
    main()
