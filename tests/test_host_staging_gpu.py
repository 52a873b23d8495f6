"""The one host staging (cj::host_batch) through its eight host entries: the same small lists with and without a caller's buffer, on one
engine, on two engines of device 0 and on one engine from two threads — equal results and bytes, the oracle's; a failed chunk keeps
the code of the single-stream export, nothing is written outside a chunk's result, the size queries give the capacities used.

The lists: b"", 1 byte, 100 bytes, 65 536, 65 537 (crosses a piece / stream boundary), a failed one, and a valid 3 000-byte one LAST,
so that the span that is copied back is decided behind a failed chunk; the first two alone (n = 2); the fourth alone (n = 1,
cj_batch_host's shortcut).  The failed one of a decoder is a stream of 2 000 bytes with the first byte flipped that the oracle
rejects; an encoder (Blosc compress, LZ4 compress against a dictionary) cannot be failed by its input, there it is a capacity of 16
bytes: the header alone.  The dictionary's encoder also refuses the chunk of 65 537 bytes (CJ_E_INPUT_TOO_LARGE): a second failed chunk."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import blosc_model as M
import lz4_dict_model as D
import oracle
from cramjam_amd import _native as N
from cramjam_amd import batch, blosc2

pytestmark = pytest.mark.gpu

DEC, ENC = N.OP_DECOMPRESS, N.OP_COMPRESS
SENTINEL = 0xA5


def _raw(n, seed):
    """half text, half noise: every container stores some of it compressed"""
    r = random.Random(seed)
    words = [b"host", b"batch", b"stage", b"span", b"scatter", b"\n"]
    out = bytearray()
    while len(out) < n // 2:
        out += r.choice(words) + b" "
    return bytes(out[:n // 2]) + r.randbytes(n - n // 2)


RAWS = [_raw(n, n) for n in (0, 1, 100, 65536, 65537, 2000, 3000)]
BAD = 5


def _blosc_chunk(raw, typesize=4, blocksize=32768):
    """a Blosc1 chunk by hand: byte shuffle, split blocks, the oracle's LZ4 streams (stored where LZ4 does not gain); below 32 bytes memcpyed"""
    n = len(raw)
    if n < 32:
        return struct.pack("<BBBBIII", 2, 1, 0x23, typesize, n, n, n + 16) + raw
    bs = min(blocksize, n)
    nblocks = (n + bs - 1) // bs
    body, table = b"", []
    for k in range(nblocks):
        blk = raw[k * bs:(k + 1) * bs]
        image = M.apply_filter(blk, typesize, M.block_mode(1, typesize, len(blk)), True)
        nsplits = typesize if len(blk) == bs else 1
        each = len(blk) // nsplits
        table.append(16 + 4 * nblocks + len(body))
        for j in range(nsplits):
            part = image[j * each:(j + 1) * each]
            comp = oracle.lz4_compress_raw(part)[1]
            if len(comp) >= each:
                comp = part
            body += struct.pack("<i", len(comp)) + comp
    return struct.pack("<BBBBIII", 2, 1, 0x21, typesize, n, bs, 16 + 4 * nblocks + len(body)) + struct.pack("<%dI" % nblocks, *table) + body


def _flipped(blob, rejected):
    """the first byte flip the oracle rejects"""
    for at in range(len(blob)):
        m = bytearray(blob)
        m[at] ^= 0xFF
        if rejected(bytes(m)):
            return bytes(m)
    raise AssertionError("no flip is rejected")


def _ptr(b):
    return C.cast(C.c_char_p(bytes(b)), C.c_void_p) if len(b) else None


def _single(fn, *extra):
    """a single-stream export as (data, cap) -> (result, bytes)"""
    def call(data, cap):
        buf = C.create_string_buffer(max(cap, 1))
        r = getattr(N.lib(), fn)(_ptr(data), len(data), C.cast(buf, C.c_void_p), cap, *extra)
        return r, buf.raw[:max(r, 0)]
    return call


PARAMS = blosc2._params(4, 5, blosc2.Filter.Shuffle, blosc2.Codec.LZ4)


class Entry:
    """one host entry: its inputs, capacities, what the oracle expects of every chunk (bytes of a decoder; None = failed), and its exports.
    bad: the chunks that fail -> the code expected (None: the single-stream export's, whatever it is)"""

    def __init__(self, name, kind, what, op, make, expect_len, single, sizes=None, size_of=None, params=None, bound=lambda n: n + 32, undo=lambda b, n: M.decode(b),
                 also_bad={}):
        self.name, self.kind, self.what, self.op, self.single, self.sizes, self.params, self.undo = name, kind, what, op, single, sizes, params, undo
        self.bad = {BAD: None, **also_bad}
        if op == DEC:
            self.inputs = [make(r) for r in RAWS]
            self.inputs[BAD] = _flipped(self.inputs[BAD], lambda m: expect_len(m, len(RAWS[BAD])) < 0)
            # the capacities: what the single-stream size export says (a raw LZ4 block has none: the oracle's length)
            self.caps = [len(RAWS[i]) if size_of is None else max(size_of(b), 0) for i, b in enumerate(self.inputs)]
        else:
            self.inputs = list(RAWS)
            self.caps = [bound(len(r)) for r in RAWS]
            self.caps[BAD] = 16                                                     # the header alone
        self.expect = [None if i in self.bad else r for i, r in enumerate(RAWS)]

    def run(self, pick, devices, out):
        ins, caps = [self.inputs[i] for i in pick], [self.caps[i] for i in pick]
        return batch._run(self.what, self.op, 0, ins, caps, devices, out, self.kind, self.params)


def _lz4_len(m, cap):
    return oracle.lz4_decompress_raw(m, cap)[0]


def _info_nbytes(b):
    info = N.BloscInfo()
    rc = N.lib().cj_blosc_chunk_info(_ptr(b), len(b), C.byref(info))
    return rc if rc != 0 else info.nbytes


DICT = D.dictionary(4096)


def _dict_stream(raw):
    """liblz4's block against DICT; the model certifies that it decodes to raw"""
    s = D.lz4_compress_with_dict(D.liblz4(), raw, DICT)
    assert D.decode(s, len(raw), DICT) == (len(raw), raw)
    return s


def _single_dict(op):
    """the chunk alone through the C export itself (cj_dict_batch_host, n = 1, marshalled by ctypes) as (data, cap) -> (result, bytes)"""
    def call(data, cap):
        data = bytes(data)
        buf = C.create_string_buffer(max(cap, 1))
        ins, lens = (C.c_void_p * 1)(C.cast(C.c_char_p(data), C.c_void_p) if data else None), (C.c_size_t * 1)(len(data))
        outs, caps, res = (C.c_void_p * 1)(C.cast(buf, C.c_void_p)), (C.c_size_t * 1)(cap), (C.c_int64 * 1)(0)
        N.check(N.lib().cj_dict_batch_host(batch._engine(0).h, N.CODEC_LZ4_BLOCK, op, 0, 1, ins, lens, outs, caps, res, C.cast(C.c_char_p(DICT), C.c_void_p), len(DICT)))
        return res[0], buf.raw[:max(res[0], 0)]
    return call


def _entries():
    L = N.lib()
    return [
        Entry("lz4_blocks", N.BLOCKS, N.CODEC_LZ4_BLOCK, DEC, lambda r: oracle.lz4_compress_raw(r)[1], _lz4_len,
              _single("cj_lz4_block_decompress", 0), batch.lz4_block_sizes),
        Entry("snappy_blocks", N.BLOCKS, N.CODEC_SNAPPY_RAW, DEC, lambda r: oracle.snappy_compress(r)[1], lambda m, cap: oracle.snappy_decompress(m, cap)[0],
              _single("cj_snappy_raw_decompress"), batch.snappy_raw_sizes, lambda b: L.cj_snappy_raw_decompress_len(_ptr(b), len(b))),
        Entry("lz4_frames", N.FRAMES, N.FORMAT_LZ4_FRAME, DEC, lambda r: oracle.lz4_frame_compress(r, 4, oracle.LZ4F_CONTENT_SIZE)[1],
              lambda m, cap: oracle.lz4_frame_decompress(m, cap)[0],
              _single("cj_lz4_frame_decompress"), batch.lz4_frame_bounds, lambda b: L.cj_lz4_frame_decompress_bound(_ptr(b), len(b))),
        Entry("snappy_framed", N.FRAMES, N.FORMAT_SNAPPY_FRAMED, DEC, lambda r: oracle.snappy_frame_compress(r)[1],
              lambda m, cap: oracle.snappy_frame_decompress(m, cap)[0],
              _single("cj_snappy_frame_decompress"), batch.snappy_framed_sizes, lambda b: L.cj_snappy_frame_decompress_len(_ptr(b), len(b))),
        Entry("blosc_decompress", N.BLOSC, 0, DEC, _blosc_chunk, lambda m, cap: 0 if M.verdict(m, cap)[0] == "ok" else -1,
              _single("cj_blosc_chunk_decompress"), batch.blosc_chunk_sizes, _info_nbytes, b""),
        Entry("blosc_compress", N.BLOSC, 0, ENC, None, None, _single("cj_blosc_chunk_compress", C.byref(PARAMS)), params=bytes(PARAMS)),
        Entry("lz4_dict_decompress", N.DICT, N.CODEC_LZ4_BLOCK, DEC, _dict_stream, lambda m, cap: D.decode(m, cap, DICT)[0], _single_dict(DEC),
              lambda blocks, devices: batch.lz4_block_sizes(blocks, devices=devices, dictionary=DICT), params=DICT),
        Entry("lz4_dict_compress", N.DICT, N.CODEC_LZ4_BLOCK, ENC, None, None, _single_dict(ENC), params=DICT,
              bound=lambda n: L.cj_lz4_block_compress_bound(n, 0), undo=lambda b, n: D.decode(b, n, DICT)[1], also_bad={4: D.INPUT_TOO_LARGE}),
    ]


NAMES = ["lz4_blocks", "snappy_blocks", "lz4_frames", "snappy_framed", "blosc_decompress", "blosc_compress", "lz4_dict_decompress", "lz4_dict_compress"]
_made = {}


def _entry(name):
    if not _made:
        for e in _entries():
            _made[e.name] = e
    return _made[name]


@pytest.fixture(scope="module")
def two_engines():
    """engine 0 and a second engine on device 0 (what a second GPU's engine would be), as tests/test_multi_gpu.py does"""
    saved = dict(batch._engines)
    batch._engines.clear()
    batch._engines[0] = saved.get(0) or N.Engine(0)
    batch._engines["second"] = N.Engine(0)
    yield
    batch._engines.pop("second").close()
    batch._engines.update(saved)


PICKS = {"all seven": list(range(7)), "the first two": [0, 1], "the fourth alone": [3]}


@pytest.mark.parametrize("pick", list(PICKS))
@pytest.mark.parametrize("name", NAMES)
def test_host_entry_every_way(name, pick, two_engines):
    e = _entry(name)
    idx = PICKS[pick]
    caps = [e.caps[i] for i in idx]
    offs = [sum(caps[:k]) for k in range(len(idx))]
    ref = None
    for devices in ([0], [0, "second"], [0, 0]):
        for into in (False, True):
            out = bytearray([SENTINEL]) * (sum(caps) + 16) if into else None
            res, outs = e.run(idx, devices, out)
            res, outs = list(res), [bytes(o) for o in outs]
            assert [len(o) for o in outs] == [max(r, 0) for r in res]
            if into:                         # nothing outside [offset, offset + max(result, 0)) of each chunk
                a = np.frombuffer(out, np.uint8)
                keep = np.ones(a.size, bool)
                for o, r in zip(offs, res):
                    keep[o:o + max(r, 0)] = False
                assert (a[keep] == SENTINEL).all(), (devices, "a write outside a chunk's result")
                for o, r, b in zip(offs, res, outs):
                    assert bytes(a[o:o + max(r, 0)]) == b
            if ref is None:
                ref = (res, outs)
            assert (res, outs) == ref, (devices, into)
    res, outs = ref
    for k, i in enumerate(idx):
        r1, o1 = e.single(e.inputs[i], e.caps[i])
        assert res[k] == r1, (i, res[k], r1)             # above all the failed chunk: the single-stream export's code
        if e.expect[i] is None:
            assert res[k] < 0 and outs[k] == b"" and e.bad[i] in (None, res[k]), (i, res[k])
        elif e.op == DEC:
            assert res[k] == len(e.expect[i]) and outs[k] == e.expect[i], i
        else:
            assert res[k] == len(outs[k]) > 0 and e.undo(outs[k], len(e.expect[i])) == e.expect[i], i


@pytest.mark.parametrize("name", [n for n in NAMES if not n.endswith("_compress")])
def test_size_queries_give_the_capacities_used(name, two_engines):
    e = _entry(name)
    one = e.sizes(e.inputs, devices=[0])
    assert one == e.sizes(e.inputs, devices=[0, "second"]) == e.sizes(e.inputs, devices=[0, 0])
    for i, s in enumerate(one):
        if i != BAD:
            assert s == e.caps[i] == len(RAWS[i]), i
        elif name not in ("lz4_blocks", "lz4_dict_decompress"):      # (the failed raw LZ4 block's capacity is not from a size export)
            assert max(s, 0) == e.caps[i], s
    assert e.sizes(e.inputs[:2], devices=[0, "second"]) == one[:2] and e.sizes(e.inputs[3:4], devices=[0, "second"]) == one[3:4]


def test_a_refused_call_reports_code_text_and_hip_text():
    """a flag bit that is not public: CJ_E_BAD_ARG from cj_batch_host itself, before any HIP call"""
    eng = batch._engine(0)
    blob = oracle.lz4_compress_raw(RAWS[2])[1]
    with pytest.raises(N.EngineError) as ex:
        eng.batch_host(N.CODEC_LZ4_BLOCK, DEC, 1 << 20, [blob], [4096])
    L = N.lib()
    assert str(ex.value) == "cramjam_hip error %d: %s (%s)" % (-101, L.cj_strerror(-101).decode(), L.cj_last_hip_error().decode())
    # ... and the same report from cj_dict_batch_host, into bytes and into a caller's buffer
    for call in (lambda: eng.batch_host(N.CODEC_LZ4_BLOCK, DEC, 1 << 20, [blob], [4096], dictionary=DICT),
                 lambda: eng.batch_host_into(N.CODEC_LZ4_BLOCK, DEC, 1 << 20, [blob], [4096], bytearray(4096), dictionary=DICT),
                 lambda: batch._run(N.CODEC_SNAPPY_RAW, DEC, 0, [blob], [4096], [0], None, N.DICT, DICT)):        # (Snappy has no dictionaries)
        with pytest.raises(N.EngineError) as ex:
            call()
        assert str(ex.value) == "cramjam_hip error %d: %s (%s)" % (-101, L.cj_strerror(-101).decode(), L.cj_last_hip_error().decode())
