"""Linked-block LZ4 frames written on the GPU (lz4_encode.hip with kFlagLinkedEnc; frame.hip: cj_lz4_frame_compress_linked,
cj_lz4_frame_compress_blocks_linked; pymod.cpp: lz4.Compressor(block_linked=True)).  The batch kernel emits the linked model's bytes
(tests/hostsim/enc2_linked_model.c) block by block; the split path and every entry point write frames the oracle reads; the default
frames stay what they were."""
import ctypes as C
import os
import random
import struct

import pytest

import oracle
from enc2_cases import cases, synth
from test_enc2_linked_model import BLOCK, corpus_streams, linked_blocks, linked_lib, model_linked

pytestmark = pytest.mark.gpu

import cramjam_amd as cramjam  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402

R = int(os.environ.get("CJ_TEST_ENC2_R", "512"))


def _call(fn, hist, data):
    L = N.lib()
    cap = len(data) + 4 * ((len(data) + BLOCK - 1) // BLOCK) + 16
    out = C.create_string_buffer(cap)
    r = fn(hist or None, len(hist), data or None, len(data), out, cap)
    assert r >= 0, (r, L.cj_strerror(r))
    return out.raw[:r]


def gpu_blocks(hist, data):
    """cj_lz4_frame_compress_blocks_linked: every block through the batch kernel, whatever the size"""
    return _call(N.lib().cj_lz4_frame_compress_blocks_linked, hist, data)


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def test_batch_kernel_emits_the_models_bytes_on_every_shape():
    L = linked_lib()
    cs = cases()
    for k, (name, raw) in enumerate(cs):
        for hist in (b"", cs[k - 1][1], synth(300 + k)[:777]):      # none, another case's tail (up to 64 KiB), a short one
            want = linked_blocks(L, raw, hist, R)
            got = gpu_blocks(hist, raw)
            assert got == want, (name, len(hist), len(got), len(want), first_diff(got, want))


def test_batch_kernel_emits_the_models_bytes_on_every_corpus_file():
    L = linked_lib()
    for name, data in corpus_streams():
        want = linked_blocks(L, data, b"", R)
        got = gpu_blocks(b"", data)
        assert got == want, (name, len(got), len(want), first_diff(got, want))


def test_every_block_of_a_batch_of_thousands_emits_the_models_bytes():
    # 2048 linked blocks in one batch (thousands of workgroups in flight); the input repeats every 24 blocks, so block k's stream is
    # the model's for (block k - 1, block k) of the period
    L = linked_lib()
    uniq = [synth(400 + i) for i in range(16)] + [c for _, chunks in corpus_streams(1 << 20) for c in [chunks[:BLOCK]]][:8]
    U = len(uniq)
    data = b"".join(uniq[i % U] for i in range(2048))
    got = gpu_blocks(b"", data)
    want = {}
    pos, k = 0, 0
    while pos < len(got):
        w = struct.unpack_from("<I", got, pos)[0]
        sz = w & 0x7FFFFFFF
        key = (k % U, k == 0)
        if key not in want:
            blk = uniq[k % U]
            c = model_linked(L, b"" if k == 0 else uniq[(k - 1) % U], blk, R)
            want[key] = (struct.pack("<I", len(blk) | 0x80000000) + blk) if len(c) >= len(blk) else struct.pack("<I", len(c)) + c
        assert got[pos:pos + 4 + sz] == want[key], (k, sz, len(want[key]))
        pos += 4 + sz
        k += 1
    assert k == 2048 and pos == len(got)


def test_linked_frames_decode_at_every_size():
    base = b"".join(synth(500 + i) for i in range(16)) + bytes(range(256)) * 64
    rnd = random.Random(5)
    for n in (0, 1, 12, 13, 8192, 8193, 65535, 65537, 1 << 20, 32 << 20, (32 << 20) + 1, 40 << 20):
        reps = n // len(base) + 1
        data = b"".join(base[rnd.randrange(0, 4096):] for _ in range(reps + 1))[:n]
        L = N.lib()
        cap = L.cj_lz4_frame_compress_bound(n)
        out = C.create_string_buffer(cap)
        r = L.cj_lz4_frame_compress_linked(data or None, n, out, cap, 4)
        assert r > 0, (n, r)
        f = out.raw[:r]
        assert f[4] == 0x44 and f[5] == 0x40, n
        rr, d = oracle.lz4_frame_decompress(f, n)
        assert rr == n and d == data, (n, rr)
        assert bytes(cramjam.lz4.decompress(f)) == data, n
        if n >= 1 << 20:                                       # repeated data: linking must shrink the frame
            ind = bytes(cramjam.lz4.compress(data))
            assert len(f) < len(ind), (n, len(f), len(ind))


def test_blocks_with_history_decode():
    # blocks_linked with a history that the first block refers to (the sizes the independent frames take the split pieces at)
    hist = b"".join(synth(600 + i) for i in range(2))
    for n in (8193, 100000, 3 << 20):
        data = (hist * (n // len(hist) + 2))[len(hist) - BLOCK + 777:][:n]       # starts inside the last 64 KiB of the history
        blocks = gpu_blocks(hist, data)
        first = struct.unpack_from("<I", blocks, 0)[0]
        assert first & 0x7FFFFFFF < min(n, BLOCK) // 4, (n, first)      # the first block is mostly a reference into the history
        hdr = bytes([0x04, 0x22, 0x4D, 0x18, 0x44, 0x40])
        hdr += bytes([(oracle.xxh32(hdr[4:6]) >> 8) & 0xFF])
        # a frame whose first flush was `hist` (as Compressor(block_linked=True) writes it)
        f = hdr + gpu_blocks(b"", hist) + blocks + struct.pack("<II", 0, oracle.xxh32(hist + data))
        rr, d = oracle.lz4_frame_decompress(f, len(hist) + n)
        assert rr == len(hist) + n and d == hist + data, (n, rr)


def test_compressor_block_linked_shrinks_a_repeated_random_block():
    # the test that needs the feature: R | R, R = random bytes — the second copy is one match into the first, across the block
    # boundary.  (R is 64 KiB - 1: a copy of EXACTLY 64 KiB lies 65536 bytes back, one more than an LZ4 offset can say — liblz4 stores
    # both blocks of that frame too.)
    r = random.Random(11).randbytes(BLOCK - 1)
    data = r + r
    outs = {}
    for bl in (True, False):
        c = cramjam.lz4.Compressor(block_linked=bl)
        c.compress(data)
        outs[bl] = bytes(c.finish())
        assert oracle.lz4_frame_decompress(outs[bl], len(data)) == (len(data), data)
    assert outs[True][4] & 0x20 == 0 and outs[False][4] & 0x20 == 0x20
    assert len(outs[True]) < 0.55 * len(outs[False]), (len(outs[True]), len(outs[False]))


def test_compressor_block_linked_streams_across_flushes():
    a = random.Random(12).randbytes(60000)
    c = cramjam.lz4.Compressor(block_linked=True)
    c.compress(a)
    f1 = bytes(c.flush())
    c.compress(a)
    f2 = bytes(c.finish())
    assert len(f2) < 400, len(f2)                    # the second copy of `a` refers to the first flush's input
    assert len(f1) > 60000
    assert oracle.lz4_frame_decompress(f1 + f2, 2 * len(a)) == (2 * len(a), a + a)
    assert bytes(cramjam.lz4.decompress(f1 + f2)) == a + a
    # many small flushes: the history is the last 64 KiB of everything before, not only the last flush
    data = b"".join(synth(700 + i) for i in range(3))
    c = cramjam.lz4.Compressor(block_linked=True, content_checksum=False)
    out = b""
    for i in range(0, len(data), 30001):
        c.compress(data[i:i + 30001])
        out += bytes(c.flush())
    c.compress(data[:70000])
    out += bytes(c.finish())
    assert oracle.lz4_frame_decompress(out, len(data) + 70000) == (len(data) + 70000, data + data[:70000])


def test_default_compressor_frames_are_unchanged():
    inputs = [b"", b"howdy neighbor", synth(800), b"".join(synth(801 + i) for i in range(5)) + b"tail", random.Random(13).randbytes(70000)]
    for data in inputs:
        want = bytes(cramjam.lz4.compress(data))              # independent blocks, FLG 0x64 (cj_lz4_frame_compress)
        assert want[4] == 0x64
        for kw in ({}, dict(block_linked=False), dict(block_linked=None)):
            c = cramjam.lz4.Compressor(**kw)
            c.compress(data)
            assert bytes(c.finish()) == want, (len(data), kw)
