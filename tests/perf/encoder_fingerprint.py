#!/usr/bin/env python3
"""Fingerprint of the GPU encoders' output on a fixed corpus (sha256 over all compressed chunks) + throughput.
Used to check that a restructured matcher still emits byte-identical streams.  GPU only."""
import hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle
from cramjam_amd import _native as N

e = N.Engine(0)
corpus = [oracle.synth_v1(65536, i) for i in range(48)]
corpus += [bytes(65536), os.urandom(0) + bytes(range(256)) * 256, b"abc" * 21845, corpus[0][:1000], corpus[1][:13], b"x" * 12, b""]
import random
random.seed(4)
corpus += [bytes(random.randrange(4) for _ in range(30000)), bytes(random.randrange(256) for _ in range(50000))]
for codec, name in ((N.CODEC_LZ4_BLOCK, "lz4"), (N.CODEC_SNAPPY_RAW, "snappy")):
    caps = [len(c) + len(c) // 6 + 64 for c in corpus]
    res, outs = e.batch_host(codec, N.OP_COMPRESS, 0, corpus, caps)
    h = hashlib.sha256()
    for r, o in zip(res, outs):
        assert r > 0 or len(o) == 0, r
        h.update(bytes(o))
    print(name, "sha256", h.hexdigest()[:16], "total", sum(res))

# The single-buffer and framed entry points (the host paths of frame.hip / large.hip): one sha256 per entry point, size and data.
# Compare a run against the library of another build (CJ_HIP_LIB) line by line.
import ctypes as C
L = N.lib()
text = b"".join(b"%d: the quick brown fox jumps over the lazy dog; %s\n" % (i, b"lorem ipsum dolor sit amet" * (i % 3)) for i in range(700000))
SIZES = [0, 1, 8192, 8193, 65536, 65537, 1 << 20, (16 << 20) + 1, 33 << 20]


def call(fn, data, cap, *extra, pre=()):
    out = C.create_string_buffer(max(cap, 1))
    r = fn(*pre, data, len(data), out, cap, *extra)
    return r, (out.raw[:r] if r > 0 else b"")


def line(name, size, kind, r, body):
    print("%-40s %9d %-6s %12d %s" % (name, size, kind, r, hashlib.sha256(body).hexdigest()[:16]), flush=True)


for size in SIZES:
    for kind, data in (("synth", oracle.synth_v1(size, 7)), ("text", text[:size])):
        assert len(data) == size
        hist = text[-100000:]
        cap = L.cj_lz4_frame_compress_bound(size) + 64
        for prep in (0, 1):
            r, z = call(L.cj_lz4_block_compress, data, L.cj_lz4_block_compress_bound(size, prep) + 64, -1, -1, prep)
            line("cj_lz4_block_compress prepend=%d" % prep, size, kind, r, z)
            if r > 0 and size:
                d = C.create_string_buffer(size)
                rd = L.cj_lz4_block_decompress(z, r, d, size, prep)
                line("cj_lz4_block_decompress prepend=%d" % prep, size, kind, rd, d.raw[:max(rd, 0)])
        r, z = call(L.cj_snappy_raw_compress, data, L.cj_snappy_raw_max_compress_len(size) + 64)
        line("cj_snappy_raw_compress", size, kind, r, z)
        if r > 0:
            d = C.create_string_buffer(max(size, 1))
            rd = L.cj_snappy_raw_decompress(z, r, d, size)
            line("cj_snappy_raw_decompress", size, kind, rd, d.raw[:max(rd, 0)])
        line("cj_snappy_frame_compress", size, kind, *call(L.cj_snappy_frame_compress, data, L.cj_snappy_frame_max_compress_len(size) + 64))
        line("cj_lz4_frame_compress", size, kind, *call(L.cj_lz4_frame_compress, data, cap, 4))
        line("cj_lz4_frame_compress_linked", size, kind, *call(L.cj_lz4_frame_compress_linked, data, cap, 4))
        line("cj_lz4_frame_compress_blocks", size, kind, *call(L.cj_lz4_frame_compress_blocks, data, cap))
        line("cj_lz4_frame_compress_blocks_linked", size, kind, *call(L.cj_lz4_frame_compress_blocks_linked, data, cap, pre=(hist, len(hist))))
