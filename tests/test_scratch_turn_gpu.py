"""One turn after another at each of an engine's seven scratches (cj::ScratchTurn, csrc/cj_engine.hpp): a small batch A and, with no wait
between them, a batch B that makes every buffer of the scratch grow while A may still be in flight — on a FRESH engine, so that the
scratch starts empty.  Metadata and results are device-resident; the engine is waited for once.  The same two batches on a second fresh
engine, each waited for, must give the same results and bytes; both are held to the oracle / the encoder's model / the recorded
fixtures, with guard bytes around every output slot.  Then B, A, B on the first engine: a turn that does not grow, and one that does
not shrink.  Closing the engines runs their teardown.  Every input is a valid stream.  (Two caller streams and two host threads on one
engine: tests/test_scratch_streams_gpu.py.)"""
import contextlib

import numpy as np
import pytest

import device_batch as DB
import lz4_dict_model as D
import oracle
import scratch_streams_cases as S
from cramjam_amd import _native as N

pytestmark = pytest.mark.gpu

FILL = DB.FILL


def _batch(stack, e, chunks, caps):
    """a batch in HBM by the harness (tests/device_batch.py): the chunks 16 bytes apart, output slot i 64 bytes behind slot i - 1's end
    in a buffer filled with FILL, the four metadata rows and the results on the device; freed when `stack` closes"""
    blob, off, lens = DB.pack(chunks, mis=0)
    ooff, total = DB.out_slots(caps)
    b = stack.enter_context(DB.device_batch(e, blob, off, lens, ooff, caps, total))
    b.ooff = [int(o) for o in ooff]
    return b


def _held_to(want, res, out, ooff):
    """chunk i produced exactly want[i] at its slot, and nothing was written outside [slot, slot + result) of any chunk"""
    assert [int(r) for r in res] == [len(w) for w in want]
    keep = np.ones(out.size, bool)
    for o, w in zip(ooff, want):
        assert out[o:o + len(w)].tobytes() == w
        keep[o:o + len(w)] = False
    assert (out[keep] == FILL).all(), "a write outside a chunk's result"


# A case: chunks(n) -> (inputs, capacities, expected outputs) of its first n chunks; enqueue(engine, batch) submits on the engine's own stream
class Blocks:
    """the workgroup decoders' scratch (cj_engine::scratch): cj_batch_device, LZ4 decompress, 256-byte word-like raws"""
    A, B = 4, 4000

    def __init__(self, flags):
        self.flags = flags
        self.raws = [D.words(256, 9000 + k) for k in range(self.B)]
        self.comp = [oracle.lz4_compress_raw(r)[1] for r in self.raws]
        assert all(oracle.lz4_decompress_raw(c, 256) == (256, r) for c, r in zip(self.comp[:8], self.raws))

    def chunks(self, n):
        return self.comp[:n], [256] * n, self.raws[:n]

    def enqueue(self, e, b):
        N.check(N.lib().cj_batch_device(e.h, N.CODEC_LZ4_BLOCK, N.OP_DECOMPRESS, self.flags, b.n, *b.args, None))


class Frames:
    """the container batches' scratch (cj_engine::fb): cj_frame_batch_device, LZ4 frames, decompress"""
    A, B = 4, 400

    def __init__(self):
        self.raws = [D.words(3000 + 7 * (k % 5), 12000 + k) for k in range(self.B)]
        self.comp = [oracle.lz4_frame_compress(r, 4, oracle.LZ4F_CONTENT_SIZE)[1] for r in self.raws]
        assert all(oracle.lz4_frame_decompress(c, len(r)) == (len(r), r) for c, r in zip(self.comp[:8], self.raws))

    def chunks(self, n):
        return self.comp[:n], [len(r) for r in self.raws[:n]], self.raws[:n]

    def enqueue(self, e, b):
        N.check(N.lib().cj_frame_batch_device(e.h, N.FORMAT_LZ4_FRAME, N.OP_DECOMPRESS, 0, b.n, *b.args, None))


class Dict:
    """the dictionary encoder's staging (cj_engine::dict_stage): cj_dict_batch_device, compress against a 4 096-byte dictionary, 300-byte chunks"""
    A, B = 4, 64

    def __init__(self):
        from test_enc2_linked_model import linked_lib, model_linked
        self.d = D.dictionary(4096)
        self.raws = [D.words(300, 15000 + k) for k in range(self.B)]
        M = linked_lib()
        self.want = [model_linked(M, self.d, r) for r in self.raws]
        assert all(D.decode(w, 300, self.d) == (300, r) for w, r in zip(self.want, self.raws))
        self.bound = N.lib().cj_lz4_block_compress_bound(300, 0)
        self.d_dict = {}

    def chunks(self, n):
        return self.raws[:n], [self.bound] * n, self.want[:n]

    def enqueue(self, e, b):
        if e not in self.d_dict:
            self.d_dict[e] = e.alloc(len(self.d))
            e.h2d(self.d_dict[e], np.frombuffer(self.d, np.uint8))
        N.check(N.lib().cj_dict_batch_device(e.h, N.CODEC_LZ4_BLOCK, N.OP_COMPRESS, 0, b.n, *b.args, self.d_dict[e], len(self.d), None))

    def free(self):
        for e, p in self.d_dict.items():
            e.free(p)


class FromCall:
    """the scratches the cases above predate, on the chunks of a call of tests/scratch_streams_cases.py that its reference accepts (at most
    `largest` bytes of capacity each), `times` times over: chunks(n) -> (inputs, capacities, their Wants)"""
    A = 4

    def __init__(self, call, kind, what, op, flags=0, times=1, largest=70000, B=None):
        rows = [(c, cap, w) for c, cap, w in zip(call.chunks, call.caps, call.want) if w.good and cap <= largest] * times
        self.rows, self.kind, self.what, self.op, self.flags = rows, kind, what, op, flags
        self.B = B or len(rows)
        assert self.A < self.B <= len(rows)

    def chunks(self, n):
        return [r[0] for r in self.rows[:n]], [r[1] for r in self.rows[:n]], [r[2] for r in self.rows[:n]]

    def enqueue(self, e, b):
        a = b.args
        N.check(getattr(N.lib(), self.kind.device)(*self.kind.device_args(e.h, self.what, self.op, self.flags, b.n, a[0:3], a[3:6], a[6], None, None)))

    @staticmethod
    def held_to(want, res, out, ooff):
        """chunk i is what want[i] says, and nothing was written outside [slot, slot + result) of any chunk"""
        keep = np.ones(out.size, bool)
        for i, (o, w) in enumerate(zip(ooff, want)):
            r = int(res[i])
            assert r >= 0 and w.problem(r, out[o:o + r]) is None, (i, w.problem(r, out[o:o + max(r, 0)]))
            keep[o:o + r] = False
        assert (out[keep] == FILL).all(), "a write outside a chunk's result"


def _small_bgzf_buffers():
    """BGZF compress: 160 buffers of a few hundred bytes (the staging of the buffers' rows grows with their number) and the call's own
    buffers of three to five members behind the first three (the member slots grow with the members of a turn)"""
    import deflate_cases as DC
    c = S.bgzf_compress()
    small = [DC.words(200 + 17 * (k % 23), 400 + k) for k in range(160)]
    bufs = small[:3] + [c.chunks[1]] + small[3:] + [x for x, w in zip(c.chunks, c.want) if w.good]
    caps = [N.lib().cj_bgzf_compress_bound(len(b)) for b in bufs]
    want = [S.Want(verify=lambda s, b=b: S._member_payloads_are_the_models(s, b)) for b in bufs]
    return S.Call("buffers into BGZF streams", "bgzf_compress_many_device", bufs, caps, want)


CASES = {
    "workgroup decoder, parse inside the decoder": lambda: Blocks(0),
    "workgroup decoder, parse kernel": lambda: Blocks(N.FLAG_FORCE_PARSE_KERNEL),
    "frame batches": Frames,
    "dictionary staging": Dict,
    # cj_engine::deflate_slots, ::zstd_slots, ::zstd_enc_slots: one slot per stream in flight, so B's 60 and more streams grow what A's four left
    "DEFLATE compress": lambda: FromCall(S.deflate_zlib_compress(), N.DEFLATE_COMPRESS, N.DEFLATE_ZLIB, N.OP_COMPRESS),
    "Zstandard decode": lambda: FromCall(S.zstd_decode(2), N.ZSTD, N.ZSTD_FRAMES, N.OP_DECOMPRESS),
    "Zstandard compress": lambda: FromCall(S.zstd_compress(0, False), N.ZSTD_COMPRESS, N.ZSTD_FRAMES, N.OP_COMPRESS),
    # cj_engine::fb through the entries that came after the frame batches: tables and pinned staging by the number of chunks, rows and
    # data scratch by their streams; the Zstandard launcher (Blosc) and the DEFLATE encoder (BGZF compress) take their turns inside
    "Blosc chunks, LZ4 streams": lambda: FromCall(S.blosc_lz4_shuffle(), N.BLOSC, 0, N.OP_DECOMPRESS, times=6),
    "BGZF decode": lambda: FromCall(S.bgzf_decode(), N.BGZF, 0, N.OP_DECOMPRESS, times=8),
    "BGZF compress": lambda: FromCall(_small_bgzf_buffers(), N.BGZF, 0, N.OP_COMPRESS, largest=1 << 30),
}


@pytest.mark.parametrize("name", list(CASES))
def test_a_turn_that_grows_the_scratch_behind_one_in_flight(name):
    case = CASES[name]()
    a, b = case.chunks(case.A), case.chunks(case.B)
    first, second = N.Engine(0), N.Engine(0)
    try:
        with contextlib.ExitStack() as stack:
            batch = lambda e, chunks: _batch(stack, e, chunks[0], chunks[1])
            # A and B back to back, one wait
            a1, b1 = batch(first, a), batch(first, b)
            case.enqueue(first, a1)
            case.enqueue(first, b1)
            first.sync()
            # ... and each waited for, on an engine of its own
            a2, b2 = batch(second, a), batch(second, b)
            case.enqueue(second, a2)
            second.sync()
            case.enqueue(second, b2)
            second.sync()
            ref = {}
            for key, x, y, chunks in (("a", a1, a2, a), ("b", b1, b2, b)):
                (rx, ox), (ry, oy) = x.read(), y.read()
                assert (rx == ry).all() and (ox == oy).all(), key
                getattr(case, "held_to", _held_to)(chunks[2], rx, ox, x.ooff)
                ref[key] = (rx, ox)
            # a turn that does not grow, then one that does not shrink
            again = [("b", batch(first, b)), ("a", batch(first, a)), ("b", batch(first, b))]
            for _, x in again:
                case.enqueue(first, x)
            first.sync()
            for key, x in again:
                r, o = x.read()
                assert (r == ref[key][0]).all() and (o == ref[key][1]).all(), key
    finally:
        if hasattr(case, "free"):
            case.free()
        first.close()
        second.close()
