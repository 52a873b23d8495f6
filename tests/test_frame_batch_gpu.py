"""Batches of framed streams on the GPU (cj_frame_batch_host / _device, cramjam_amd.batch.*_frames / *_framed_many): every stream's
result and bytes equal the single-stream export's (cj_lz4_frame_decompress / cj_snappy_frame_decompress with the same capacity) —
errors and their stream-order precedence included — and compressed frames are assembled from exactly the block batch's payloads."""
import base64
import ctypes as C
import json
import os
import random
import struct

import numpy as np
import pytest

import device_batch as DB
import oracle
import cramjam_amd as cj
from cramjam_amd import _native as N
from cramjam_amd import batch
from framing import SNAPPY_IDENT, crc32c_masked, snappy_chunk, snappy_compressed, snappy_stored

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GUARD = 0xA5


def _text(n, seed):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"frame", b"batch", b"stream", b"block", b"\n"]
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def _rand(n, seed):
    return random.Random(seed).randbytes(n)


def _single(fmt, frame, cap):
    L = N.lib()
    fn = L.cj_lz4_frame_decompress if fmt == N.FORMAT_LZ4_FRAME else L.cj_snappy_frame_decompress
    buf = C.create_string_buffer(max(cap, 1))
    b = bytes(frame)
    r = fn(C.cast(C.c_char_p(b), C.c_void_p) if b else None, len(b), C.cast(buf, C.c_void_p), cap)
    return r, buf.raw[:max(r, 0)]


def _batch_guarded(fmt, frames, caps):
    """host batch into one buffer with 16 guard bytes between the slots; returns results, outputs, and whether every guard is intact"""
    offs, run = [], 16
    for c in caps:
        offs.append(run); run += c + 16
    out = np.full(run + 16, GUARD, np.uint8)
    eng = batch._engine(0)
    res = eng.batch_host_into(fmt, N.OP_DECOMPRESS, 0, frames, caps, out, offs, "cj_frame_batch_host")
    mask = np.ones(out.size, bool)
    for o, c in zip(offs, caps):
        mask[o:o + c] = False
    outs = [bytes(out[o:o + max(r, 0)]) for o, r in zip(offs, res)]
    return res, outs, bool((out[mask] == GUARD).all())


def _lz4_frames():
    g = json.load(open(os.path.join(GOLDEN, "golden_frames.json")))
    frames = [base64.b64decode(v["frame"]) for v in g["vectors"]]
    L = N.lib()
    for i, n in enumerate([0, 1, 100, 8192, 65535, 65536, 65537, 200000, 600000]):
        d = _text(n, i) if i % 2 else _rand(n, i)
        frames.append(bytes(cj.lz4.compress(d)))
        cap = L.cj_lz4_frame_compress_bound(n)
        buf = C.create_string_buffer(max(cap, 1))
        r = L.cj_lz4_frame_compress_linked(d, n, C.cast(buf, C.c_void_p), cap, 0)
        assert r > 0
        frames.append(buf.raw[:r])
        for bs, fl in ((4, 0), (5, oracle.LZ4F_LINKED), (6, oracle.LZ4F_BLOCK_CHECKSUM | oracle.LZ4F_CONTENT_SIZE), (7, oracle.LZ4F_NO_CONTENT_CHECKSUM)):
            if n <= 200000 or bs == 4:
                frames.append(oracle.lz4_frame_compress(d, bs, fl)[1])
    for linked, csum in ((True, True), (False, False)):
        c = cj.lz4.Compressor(block_linked=linked, content_checksum=csum)
        parts = []
        for k in range(3):
            c.compress(_text(70000 + 1000 * k, 50 + k))
            parts.append(bytes(c.flush()))
        parts.append(bytes(c.finish()))
        frames.append(b"".join(parts))
    frames.append(struct.pack("<II", 0x184D2A53, 5) + b"skip!")          # skippable
    frames.append(frames[-1] + frames[0])                                  # bytes after the first frame are ignored
    frames.append(open(os.path.join(GOLDEN, "plaintext.txt.lz4"), "rb").read())
    return frames


def _snappy_streams():
    streams = []
    for i, n in enumerate([0, 1, 100, 65535, 65536, 65537, 300000]):
        d = _text(n, 100 + i) if i % 2 else _rand(n, 100 + i)
        streams.append(bytes(cj.snappy.compress(d)))
        streams.append(oracle.snappy_frame_compress(d)[1])
    p1, p2 = _text(3000, 1), _text(70000, 2)[:65536]
    streams.append(SNAPPY_IDENT + snappy_chunk(0xfe, b"\0" * 7) + snappy_stored(p1) + snappy_chunk(0x80, b"xyz") + SNAPPY_IDENT
                   + snappy_compressed(p2, oracle.snappy_compress(p2)[1]) + snappy_stored(b""))
    streams.append(SNAPPY_IDENT + SNAPPY_IDENT + snappy_stored(_rand(65536, 3)))
    streams.append(open(os.path.join(GOLDEN, "plaintext.txt.snappy"), "rb").read())
    return streams


def _check_against_single(fmt, frames, caps=None):
    if caps is None:
        L = N.lib()
        bound = L.cj_lz4_frame_decompress_bound if fmt == N.FORMAT_LZ4_FRAME else L.cj_snappy_frame_decompress_len
        caps = [max(bound(f, len(f)), 0) if f else 0 for f in frames]
    res, outs, guards = _batch_guarded(fmt, frames, caps)
    assert guards, "a write outside a slot"
    for i, (f, c) in enumerate(zip(frames, caps)):
        r1, o1 = _single(fmt, f, c)
        assert res[i] == r1, (i, len(f), c, res[i], r1)
        if r1 >= 0:
            assert outs[i] == o1, i
    return res, outs, caps


def test_lz4_frames_batch_matches_single_calls_and_oracle():
    frames = _lz4_frames()
    res, outs, _ = _check_against_single(N.FORMAT_LZ4_FRAME, frames)
    assert min(res) >= 0
    for f, r, o in zip(frames, res, outs):
        rr, oo = oracle.lz4_frame_decompress(f)
        assert (rr, oo) == (r, o)
    r2, o2 = batch.lz4_decompress_frames(frames)
    assert r2 == res and [bytes(x) for x in o2] == outs


def test_snappy_streams_batch_matches_single_calls_and_oracle():
    streams = _snappy_streams()
    res, outs, _ = _check_against_single(N.FORMAT_SNAPPY_FRAMED, streams)
    assert min(res) >= 0
    for s, r, o in zip(streams, res, outs):
        assert oracle.snappy_frame_decompress(s) == (r, o)
    r2, o2 = batch.snappy_decompress_framed_many(streams)
    assert r2 == res and [bytes(x) for x in o2] == outs


def _lz4_mutants(f, rnd):
    out = []
    if len(f) < 12 or f[:4] != b"\x04\x22\x4d\x18":
        return out
    flg = f[4]
    hl = 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    m = bytearray(f); m[hl] ^= 0x01; out.append(bytes(m))                   # header checksum
    m = bytearray(f); m[4] |= 0x02; out.append(bytes(m))                    # reserved bit
    m = bytearray(f); m[5] = 0x30; out.append(bytes(m))                     # block-size code 3
    m = bytearray(f); m[hl + 1:hl + 5] = struct.pack("<I", 0x7FFFFFFF); out.append(bytes(m))       # block word above block_max
    w = struct.unpack("<I", f[hl + 1:hl + 5])[0]
    for cut in sorted({hl, hl + 1, hl + 3, hl + 5, hl + 5 + (w & 0x7FFFFFFF) // 2, len(f) - 9, len(f) - 5, len(f) - 4, len(f) - 1}):
        if 0 <= cut < len(f):
            out.append(f[:cut])                                             # truncations at structural offsets
    if w and not w & 0x80000000 and (w & 0x7FFFFFFF) > 8:
        m = bytearray(f); m[hl + 5 + 1] ^= 0xFF; m[hl + 5 + 2] = 0xF0; out.append(bytes(m))         # bad block body
    if flg & 0x10 and w:
        m = bytearray(f); m[hl + 5 + (w & 0x7FFFFFFF)] ^= 1; out.append(bytes(m))                  # block checksum
    if flg & 0x04:
        m = bytearray(f); m[-1] ^= 0x40; out.append(bytes(m))               # content checksum
    m = bytearray(f); m[rnd.randrange(hl + 5, len(f))] ^= 1 << rnd.randrange(8); out.append(bytes(m))
    return out


def _snappy_mutants(s, rnd):
    out = []
    if len(s) < 18:
        return out
    m = bytearray(s); m[14] ^= 1; out.append(bytes(m))                     # CRC of the first data chunk
    m = bytearray(s); m[10] = 0x02; out.append(bytes(m))                   # reserved unskippable chunk type
    m = bytearray(s); m[11:14] = b"\xff\xff\x00"; out.append(bytes(m))     # chunk length
    m = bytearray(s); m[0] = 0x00; out.append(bytes(m))                    # no stream identifier
    for cut in (3, 10, 12, 16, 20, len(s) // 2, len(s) - 1):
        if cut < len(s):
            out.append(s[:cut])
    m = bytearray(s); m[rnd.randrange(18, len(s))] ^= 1 << rnd.randrange(8); out.append(bytes(m))
    return out


@pytest.mark.parametrize("fmt", [N.FORMAT_LZ4_FRAME, N.FORMAT_SNAPPY_FRAMED])
def test_corrupt_streams_keep_the_single_call_verdict_and_spare_their_neighbours(fmt):
    rnd = random.Random(1234)
    good = _lz4_frames() if fmt == N.FORMAT_LZ4_FRAME else _snappy_streams()
    mut = _lz4_mutants if fmt == N.FORMAT_LZ4_FRAME else _snappy_mutants
    frames, caps = [], []
    L = N.lib()
    bound = L.cj_lz4_frame_decompress_bound if fmt == N.FORMAT_LZ4_FRAME else L.cj_snappy_frame_decompress_len
    for f in good:
        c = max(bound(f, len(f)), 0) if f else 0
        frames.append(f); caps.append(c)                                    # an intact neighbour before every group
        for m in mut(f, rnd):
            frames.append(m); caps.append(c)
        r1, o1 = _single(fmt, f, c)
        if r1 > 0:
            frames.append(f); caps.append(r1 - 1)                           # one byte short
    assert len(frames) > 150
    res, _, _ = _check_against_single(fmt, frames, caps)
    assert any(r < 0 for r in res) and any(r > 0 for r in res)


def _lz4_frame_by_hand(blocks, bd=0x70, flg=0x60):
    """an LZ4 frame of the given (word, payload) blocks, no checksums: written by the format, not by a compressor"""
    hc = (oracle.xxh32(bytes([flg, bd])) >> 8) & 0xFF
    return b"\x04\x22\x4d\x18" + bytes([flg, bd, hc]) + b"".join(struct.pack("<I", w) + p for w, p in blocks) + b"\0\0\0\0"


def test_many_small_blocks_of_4mib_frames_do_not_reserve_block_max_each():
    # 200 000 stored 1-byte blocks of a frame with 4 MiB blocks: the decode scratch follows what the blocks can produce, not block_max per
    # block (that would be 781 GiB and fail the whole batch); the same for many tiny compressed blocks, independent and linked
    stored = _lz4_frame_by_hand([(1 | 0x80000000, bytes([65 + k % 26])) for k in range(200000)])
    tiny = [(2, b"\x10" + bytes([97 + k % 26])) for k in range(300)]           # one literal each
    comp = _lz4_frame_by_hand(tiny)
    linked = _lz4_frame_by_hand(tiny[:64] + [(0x80000000 | 3, b"xyz")], flg=0x40)
    bad = _lz4_frame_by_hand(tiny[:100] + [(2, b"\xf0\x00")] + tiny[:5])    # a malformed block among them
    good = _lz4_frames()[:40]
    frames = good[:20] + [stored, comp, linked, bad] + good[20:]
    res, outs, _ = _check_against_single(N.FORMAT_LZ4_FRAME, frames)
    assert res[20:24] == [200000, 300, 67, -27], res[20:24]
    assert outs[20] == bytes(65 + k % 26 for k in range(200000))
    assert outs[21] == bytes(97 + k % 26 for k in range(300))


def test_xxh32_kernel_matches_the_algorithm_at_every_alignment():
    eng = batch._engine(0)
    data = _rand(4 << 20, 77)
    offs, lens = [], []
    for a in range(16):
        for n in range(301):
            offs.append(4096 + a); lens.append(n)
    for a in range(16):
        for n in (1023, 1024, 1025, 2047, 4096 + 7, 70001):
            offs.append(8192 + a); lens.append(n)
    offs += [3, 1 << 20]; lens += [(3 << 20) + 5, (2 << 20) + 13]
    L = N.lib()
    d_in = eng.alloc(len(data) + 64)
    d_off, d_len, d_out = eng.alloc(8 * len(offs)), eng.alloc(8 * len(offs)), eng.alloc(4 * len(offs))
    try:
        eng.h2d(d_in, np.frombuffer(data, np.uint8))
        eng.h2d(d_off, np.array(offs, np.uint64)); eng.h2d(d_len, np.array(lens, np.uint64))
        N.check(L.cj_debug_xxh32_device(eng.h, d_in, d_off, d_len, d_out, len(offs)))
        got = eng.d2h(d_out, 4 * len(offs), "uint32")
    finally:
        for p in (d_in, d_off, d_len, d_out):
            eng.free(p)
    for k, (o, n) in enumerate(zip(offs, lens)):
        assert int(got[k]) == oracle.xxh32(data[o:o + n]), (o, n)


def _lz4_frame_from_blocks(d):
    pieces = [d[k:k + 65536] for k in range(0, len(d), 65536)]
    res, outs = batch.lz4_compress_blocks(pieces, store_size=False) if pieces else ([], [])
    hc = (oracle.xxh32(b"\x64\x40") >> 8) & 0xFF
    f = b"\x04\x22\x4d\x18\x64\x40" + bytes([hc])
    for p, r, o in zip(pieces, res, outs):
        assert r > 0
        f += struct.pack("<I", len(p) | 0x80000000) + p if r >= len(p) else struct.pack("<I", r) + bytes(o)
    return f + struct.pack("<II", 0, oracle.xxh32(d))


def _snappy_stream_from_blocks(d):
    if not d:
        return b""
    pieces = [d[k:k + 65536] for k in range(0, len(d), 65536)]
    res, outs = batch.snappy_compress_raw_many(pieces)
    s = SNAPPY_IDENT
    for p, r, o in zip(pieces, res, outs):
        s += snappy_stored(p) if r >= len(p) - len(p) // 8 else snappy_compressed(p, bytes(o))
    return s


def test_compressed_frames_are_the_block_batch_payloads():
    inputs = []
    for i, n in enumerate([0, 1, 100, 4096, 8192, 65535, 65536, 65537, 3 << 20]):
        inputs.append(_rand(n, 300 + i)); inputs.append(_text(n, 400 + i))
    r4, o4 = batch.lz4_compress_frames(inputs)
    rs, os_ = batch.snappy_compress_framed_many(inputs)
    for i, d in enumerate(inputs):
        assert bytes(o4[i]) == _lz4_frame_from_blocks(d), (i, len(d))
        assert bytes(os_[i]) == _snappy_stream_from_blocks(d), (i, len(d))
        assert oracle.lz4_frame_decompress(bytes(o4[i])) == (len(d), d)
        assert oracle.snappy_frame_decompress(bytes(os_[i])) == (len(d), d)
        if len(d) <= 8192:
            assert bytes(o4[i]) == bytes(cj.lz4.compress(d)) and bytes(os_[i]) == bytes(cj.snappy.compress(d)), len(d)
    assert r4[0] == 15 and rs[0] == 0


def test_compress_capacity_too_small_is_a_write_error_with_no_write():
    eng = batch._engine(0)
    d = [_text(5000, 1), _rand(70000, 2)]
    for fmt, single in ((N.FORMAT_LZ4_FRAME, cj.lz4.compress), (N.FORMAT_SNAPPY_FRAMED, cj.snappy.compress)):
        sizes = [len(bytes(single(x))) for x in d]
        caps = [sizes[0] - 1, sizes[1]]
        out = np.full(sum(caps) + 64, GUARD, np.uint8)
        res = eng.batch_host_into(fmt, N.OP_COMPRESS, 0, d, caps, out, [16, 32 + caps[0]], "cj_frame_batch_host")
        assert res[0] == -14 and res[1] > 0
        assert (out[:32 + caps[0]] == GUARD).all()


def test_device_resident_frame_batches_from_torch_tensors():
    pytest.importorskip("torch")
    DB.run_child(os.path.join(HERE, "frame_batch_child.py"), "frame batch device: ok", 900)
