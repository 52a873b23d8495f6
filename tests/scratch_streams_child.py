"""Child process of tests/test_scratch_streams_gpu.py: two caller streams and two host threads on the ONE cached engine of device 0,
one pairing per shared scratch of cj_engine (tests/scratch_streams_cases.py lists them and says where the inputs and the expected
bytes come from).  Call X goes to stream `a`, call Y to stream `b`, through the cramjam_amd.batch.*_device entries with sync=False;
metadata and results are device tensors, every output buffer is filled with 0xA5 and has 64 guard bytes around every slot, and the
budget that governs the pairing's scratch is lowered to three slots, so both calls run many slices over the same few slots.

Per pairing: ALONE (X, wait, Y, wait — held to the references on the host, and timed: X's device time between two events, the host
cost of submitting Y); INTERLEAVED (X(a), Y(b) four times over from one thread, each into buffers of its own, one synchronisation of
both streams); THREADS (thread 1 loops X on `a`, thread 2 loops Y on `b`, behind a barrier); for P1 and P5 a HOST batch in thread 1
beside the device batch in thread 2.  Every result row and every output byte of the later modes equals the alone run's (compared on
the device; copied back only on a mismatch).  Arguments: the names of the pairings to run (default: all).

torch is imported BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys
import threading
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import scratch_streams_cases as S  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

ROUNDS = 4


class Dev:
    """a Call in HBM: its input and its four metadata rows as device tensors (uploaded once, read-only), and the stream it goes to"""

    def __init__(self, call, stream):
        self.call, self.stream = call, stream
        size, off, ln, self.ooff, self.total = call.layout()
        blob = np.zeros(size, np.uint8)
        for o, c in zip(off, call.chunks):
            blob[o:o + len(c)] = np.frombuffer(c, np.uint8)
        self.t_in = torch.from_numpy(blob).cuda()
        self.meta = [torch.tensor(row, dtype=torch.int64).cuda() for row in (off, ln, self.ooff, call.caps)]
        self.t_dict = torch.from_numpy(np.frombuffer(call.dictionary, np.uint8).copy()).cuda() if call.dictionary is not None else None
        torch.cuda.synchronize()

    def fresh(self):
        """(output, result) of one submission: 0xA5 everywhere, results that no call gives"""
        return (torch.full((self.total,), S.FILL, dtype=torch.uint8, device="cuda"), torch.full((self.call.n,), -0x7777, dtype=torch.int64, device="cuda"))

    def submit(self, bufs):
        out, res = bufs
        c, h = self.call, self.stream.cuda_stream
        if c.flags:                       # a flag Python does not expose: the C entry on the tensors' addresses
            eng = batch._engine(0)
            N.check(N.lib().cj_batch_device(eng.h, c.codec, N.OP_DECOMPRESS, c.flags, c.n, self.t_in.data_ptr(), self.meta[0].data_ptr(), self.meta[1].data_ptr(),
                                            out.data_ptr(), self.meta[2].data_ptr(), self.meta[3].data_ptr(), res.data_ptr(), h))
            return
        kw = dict(c.kw)
        if self.t_dict is not None:
            kw["dictionary"] = self.t_dict
        got = getattr(batch, c.entry)(self.t_in, self.meta[0], self.meta[1], out, self.meta[2], self.meta[3], result=res, stream=h, sync=False, **kw)
        assert got is res

    def host(self):
        """the call through its host entry: (results, outputs as bytes)"""
        c = self.call
        if c.host == "lz4_decompress_blocks":
            res, outs = batch.lz4_decompress_blocks(c.chunks, output_lens=c.caps)
        else:
            res, outs = getattr(batch, c.host)(c.chunks)
        return [int(r) for r in res], [bytes(o) for o in outs]


def first_difference(dev, got, ref):
    """where two (output, result) pairs of one Dev differ: copied back for the message"""
    (o1, r1), (o2, r2) = [(o.cpu().numpy(), r.cpu().numpy()) for o, r in (got, ref)]
    rows = np.flatnonzero(r1 != r2)
    if rows.size:
        return "result row %d: %d, alone %d" % (rows[0], r1[rows[0]], r2[rows[0]])
    at = int(np.flatnonzero(o1 != o2)[0])
    i = max([k for k, o in enumerate(dev.ooff) if o - S.G <= at], default=0)
    return "chunk %d, byte %d of its slot (capacity %d): 0x%02x, alone 0x%02x" % (i, at - dev.ooff[i], dev.call.caps[i], o1[at], o2[at])


def same(dev, got, ref, what):
    if not (torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])):
        raise AssertionError("%s, %s: %s" % (what, dev.call.label, first_difference(dev, got, ref)))


def alone(dev):
    """one warm-up (the scratch grows, the kernels load), then the run that counts: ((output, result), device ms, host ms of the submission)"""
    warm, bufs = dev.fresh(), dev.fresh()
    torch.cuda.synchronize()
    dev.submit(warm)
    dev.stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(dev.stream)
    t0 = time.perf_counter()
    dev.submit(bufs)
    host_ms = (time.perf_counter() - t0) * 1e3
    e1.record(dev.stream)
    dev.stream.synchronize()
    bad = dev.call.problems(bufs[1].cpu().numpy(), bufs[0].cpu().numpy(), dev.ooff)
    assert not bad, "alone, %s: %d chunks off the reference, first %r" % (dev.call.label, len(bad), bad[:3])
    return bufs, e0.elapsed_time(e1), host_ms


def in_threads(*loops):
    """every loop in a thread of its own behind one barrier; the first exception of any of them is raised here"""
    gate, errors = threading.Barrier(len(loops)), []

    def run(fn):
        try:
            gate.wait(timeout=120)
            fn()
        except BaseException as ex:      # noqa: B036 (handed to the parent thread)
            errors.append(ex)
            gate.abort()
    ts = [threading.Thread(target=run, args=(fn,)) for fn in loops]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errors:
        raise errors[0]


def run_pairing(p, a, b):
    L = N.lib()
    prev = [(name, getattr(L, name)(nbytes)) for name, nbytes in p.budgets]
    try:
        X, Y = Dev(p.x, a), Dev(p.y, b)
        x0, x_ms, _ = alone(X)
        y0, y_ms, y_submit = alone(Y)
        factor = x_ms / y_submit
        line = "%s [%s] X %s: %.3f ms alone on the device; Y %s: %.3f ms to submit, %.3f ms on the device; X / submit(Y) = %.1f%s" % (
            p.name, p.scratch, p.x.label, x_ms, p.y.label, y_submit, y_ms, factor, "" if factor >= 10 else " (BELOW 10)")
        # one host thread, the calls interleaved
        xs, ys = [X.fresh() for _ in range(ROUNDS)], [Y.fresh() for _ in range(ROUNDS)]
        torch.cuda.synchronize()
        for bx, by in zip(xs, ys):
            X.submit(bx)
            Y.submit(by)
        a.synchronize(); b.synchronize()
        for k, (bx, by) in enumerate(zip(xs, ys)):
            same(X, bx, x0, "%s interleaved, round %d" % (p.name, k))
            same(Y, by, y0, "%s interleaved, round %d" % (p.name, k))
        # two host threads
        xs, ys = [X.fresh() for _ in range(ROUNDS)], [Y.fresh() for _ in range(ROUNDS)]
        torch.cuda.synchronize()
        in_threads(lambda: [X.submit(bx) for bx in xs], lambda: [Y.submit(by) for by in ys])
        a.synchronize(); b.synchronize()
        for k, (bx, by) in enumerate(zip(xs, ys)):
            same(X, bx, x0, "%s threads, round %d" % (p.name, k))
            same(Y, by, y0, "%s threads, round %d" % (p.name, k))
        line += "; alone, interleaved, threads ok"
        if p.host_mode:
            # a host batch (staged under the engine's mutex, on the engine's stream) beside a device batch on `b`
            H = X if p.x.host else Y
            h0 = H.host()
            for i, w in enumerate(H.call.want):
                if w.good:
                    assert w.problem(h0[0][i], h0[1][i]) is None, ("host batch alone", H.call.label, i, w.problem(h0[0][i], h0[1][i]))
                else:
                    assert h0[0][i] < 0, ("host batch alone", H.call.label, i, h0[0][i])
            ys, hs = [Y.fresh() for _ in range(ROUNDS)], []
            torch.cuda.synchronize()
            in_threads(lambda: [hs.append(H.host()) for _ in range(ROUNDS)], lambda: [Y.submit(by) for by in ys])
            b.synchronize()
            for k, by in enumerate(ys):
                same(Y, by, y0, "%s host beside device, round %d" % (p.name, k))
                assert hs[k] == h0, "%s host beside device, round %d: the host batch differs from its alone run" % (p.name, k)
            line += ", host beside device ok"
        print(line, flush=True)
    finally:
        for name, old in prev:
            getattr(L, name)(old)


def main(names):
    ps = S.pairings()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    t0 = time.perf_counter()
    for name in names or list(ps):
        t1 = time.perf_counter()
        run_pairing(ps[name], a, b)
        print("%s: %.1f s" % (name, time.perf_counter() - t1), flush=True)
    torch.cuda.synchronize()
    print("scratch streams: ok, %d pairings, %.1f s" % (len(names or ps), time.perf_counter() - t0))


if __name__ == "__main__":
    main(sys.argv[1:])
