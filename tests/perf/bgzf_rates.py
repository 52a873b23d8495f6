"""Rates and ratios of the BGZF batches on one MI355X.  Device-resident, HIP events, a warm-up and the median of RUNS
runs with min .. max.  torch is imported first (one HIP runtime per process).  Prints one JSON line per figure.
  python tests/perf/bgzf_rates.py [--quick] [--decode | --encode]      (--quick: one pass at a sixteenth of the size)
Decode: ONE stream of 16 384 members of 65 280 text-like bytes (the two walk passes are two serial hop chains on one lane), and 16 384
streams of one such member, each against cj_deflate_batch_device (gzip) over the same members pre-split — the kernels of the DEFLATE
batches, which the BGZF path launches unchanged.  Encode: one buffer of 16 384 x 65 280 bytes (1 GiB less 4 MiB) through the BGZF
encoder against cj_deflate_compress_batch_device (gzip) over the same buffer as ONE chunk (one workgroup; timed on a prefix when a
full run would take minutes: the line says so) and over the same 65 280-byte pieces as a batch.
The kernels' own times (the walk passes bgzf_count_kernel / bgzf_rows_kernel, the assembly bgzf_layout_kernel / bgzf_assemble_kernel /
piece_rows_kernel<BgEnc>) come from a kernel trace of a --quick run: rocprofv3 --kernel-trace --stats -- python tests/perf/bgzf_rates.py --quick"""
import json
import os
import statistics
import struct
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deflate_cases as D  # noqa: E402
from cramjam_amd import batch  # noqa: E402

QUICK = "--quick" in sys.argv
RUNS = 1 if QUICK else 9
PIECE = 65280
MEMBERS = 16384 // (16 if QUICK else 1)
dev = torch.device("cuda:0")


def say(**kw):
    print(json.dumps(kw), flush=True)


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), runs=len(ms))


def timed(fn, side, runs=None):
    ev = []
    for k in range((RUNS if runs is None else runs) + 1):
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


def main():
    side = torch.cuda.Stream()
    s = side.cuda_stream
    uniq = [D.words(PIECE, 7000 + k) for k in range(64)]
    total = MEMBERS * PIECE
    kw = dict(stream=s, sync=False)
    with torch.cuda.stream(side):
        raw = torch.from_numpy(np.frombuffer(b"".join(uniq), np.uint8).copy()).to(dev).repeat(MEMBERS // len(uniq))
        raw = torch.cat([raw, torch.zeros(64, dtype=torch.uint8, device=dev)])
        cap = batch.bgzf_compress_bound(total)
        comp = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        one_off, one_len, one_cap, one_res = i64([0]), i64([total]), i64([cap]), torch.empty(1, dtype=torch.int64, device=dev)
        back = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    side.synchronize()

    # ---- encode: one buffer, one BGZF stream
    enc = lambda: batch.bgzf_compress_many_device(raw, one_off, one_len, comp, one_off, one_cap, result=one_res, **kw)
    ev_enc = timed(enc, side) if "--decode" not in sys.argv else (enc(), side.synchronize(), [float("nan")])[2]
    size = int(one_res.cpu()[0])
    assert size > 0
    head = comp[:size].cpu().numpy().tobytes()
    # the member rows, from a walk on the host (the yardsticks get the members pre-split)
    mem, pos = [], 0
    while pos < size:
        ln = struct.unpack_from("<H", head, pos + 16)[0] + 1
        mem.append((pos, ln))
        pos += ln
    assert len(mem) == MEMBERS + 1 and mem[-1][1] == 28
    mem = mem[:-1]
    m_off, m_len = i64([m[0] for m in mem]), i64([m[1] for m in mem])
    p_off, p_len = i64(np.arange(MEMBERS) * PIECE), i64(np.full(MEMBERS, PIECE))
    m_res = torch.empty(MEMBERS, dtype=torch.int64, device=dev)

    if "--decode" not in sys.argv:
        bgzf = statistics.median(ev_enc)
        say(what="encode: one buffer of %d x %d B into one BGZF stream" % (MEMBERS, PIECE), GBps=round(total / bgzf / 1e6, 2), ratio=round(total / size, 3), **stats(ev_enc))
        stride = (batch.deflate_compress_bound(PIECE, "gzip") + 15) // 16 * 16
        with torch.cuda.stream(side):
            c_off, c_cap = i64(np.arange(MEMBERS) * stride), i64(np.full(MEMBERS, stride))
            pieces = torch.empty(MEMBERS * stride + 64, dtype=torch.uint8, device=dev)
        ev = timed(lambda: batch.deflate_compress_many_device(raw, p_off, p_len, pieces, c_off, c_cap, wrapper="gzip", result=m_res, **kw), side)
        assert int(m_res.min()) > 0 and int(m_res.sum()) + 8 * MEMBERS + 28 == size
        as_batch = statistics.median(ev)
        say(what="encode yardstick: the same %d pieces as a gzip batch" % MEMBERS, GBps=round(total / as_batch / 1e6, 2), bgzf_over_it=round(bgzf / as_batch, 3),
            container_share_of_bgzf=round(1 - as_batch / bgzf, 3), **stats(ev))
        del pieces
        # the same buffer as ONE gzip chunk: one workgroup.  A prefix first; the whole buffer only if that takes seconds, not minutes
        prefix = min(total, 64 * PIECE)
        cap1 = batch.deflate_compress_bound(total, "gzip")
        with torch.cuda.stream(side):
            one = torch.empty(cap1 + 64, dtype=torch.uint8, device=dev)
        def run1(n):
            ln, cp = i64([n]), i64([cap1])
            return lambda: batch.deflate_compress_many_device(raw, one_off, ln, one, one_off, cp, wrapper="gzip", result=one_res, **kw)
        ev = timed(run1(prefix), side, 1)
        n1, runs1 = (total, 3) if ev[-1] * (total / prefix) * 4 < 60000 else (prefix, RUNS)
        if n1 != prefix:
            ev = timed(run1(n1), side, runs1)
        assert int(one_res.cpu()[0]) > 0
        single = statistics.median(ev) * (total / n1)
        say(what="encode yardstick: the buffer as ONE gzip chunk (one workgroup), timed on %d B%s" % (n1, "" if n1 == total else ", scaled to the whole buffer"),
            GBps=round(n1 / statistics.median(ev) / 1e6, 3), bgzf_is_faster_by=round(single / bgzf, 1), **stats(ev))
        del one
    if "--encode" in sys.argv:
        return

    # ---- decode
    with torch.cuda.stream(side):
        one_clen, out_cap1 = i64([size]), i64([total])
    ev = timed(lambda: batch.deflate_decompress_many_device(comp, m_off, m_len, back, p_off, p_len, wrapper="gzip", result=m_res, **kw), side)
    assert int(m_res.min()) == PIECE and torch.equal(back[:total], raw[:total])
    base = statistics.median(ev)
    say(what="decode yardstick: %d gzip members pre-split (cj_deflate_batch_device)" % MEMBERS, GBps=round(total / base / 1e6, 2), **stats(ev))
    back.zero_()
    ev = timed(lambda: batch.bgzf_decompress_many_device(comp, one_off, one_clen, back, one_off, out_cap1, result=one_res, **kw), side)
    assert int(one_res.cpu()[0]) == total and torch.equal(back[:total], raw[:total])
    t = statistics.median(ev)
    say(what="decode: ONE stream of %d members" % MEMBERS, GBps=round(total / t / 1e6, 2), over_presplit=round(t / base, 3), **stats(ev))
    back.zero_()
    ev = timed(lambda: batch.bgzf_decompress_many_device(comp, m_off, m_len, back, p_off, p_len, result=m_res, **kw), side)
    assert int(m_res.min()) == PIECE and torch.equal(back[:total], raw[:total])
    t = statistics.median(ev)
    say(what="decode: %d streams of one member" % MEMBERS, GBps=round(total / t / 1e6, 2), over_presplit=round(t / base, 3), **stats(ev))
    ev = timed(lambda: batch.bgzf_sizes_device(comp, one_off, one_clen, result=one_res, **kw), side)
    assert int(one_res.cpu()[0]) == total
    say(what="size query: ONE stream of %d members (one walk pass on one lane)" % MEMBERS, us_per_hop=round(statistics.median(ev) * 1e3 / (MEMBERS + 1), 3), **stats(ev))


if __name__ == "__main__":
    main()
