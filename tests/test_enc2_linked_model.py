"""The linked-block mode of the LZ4 encoder, stated as scalar C (tests/hostsim/enc2_linked_model.c: what lz4_encode.hip computes with
kFlagLinkedEnc): with no history it is the independent model, its frames (FLG 0x44) decode with the oracle, and linking buys what the
stream format promises — never a byte more per file of the reference's corpus, 3 % or more in total, and within 8 % of liblz4's own
linked frames.  CPU only; tests/test_linked_frames_gpu.py holds the kernel to these bytes."""
import bz2
import ctypes as C
import json
import os
import struct
import subprocess

import oracle
from conftest import ROOT
from enc2_cases import cases
from test_enc2_model import corpus_files, model_lib, model_lz4

SIM_DIR = os.path.join(ROOT, "tests", "hostsim")
SIM_SO = os.path.join(SIM_DIR, "libsim_enc2_linked.so")
BLOCK = 65536


def linked_lib():
    srcs = [os.path.join(SIM_DIR, f) for f in ("enc2_linked_model.c", "enc2_model.c", "enc2_round.h")]
    if not os.path.exists(SIM_SO) or os.path.getmtime(SIM_SO) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-o", SIM_SO, srcs[0]])
    L = C.CDLL(SIM_SO)
    L.enc2_model_lz4_linked.restype = C.c_int64
    L.enc2_model_lz4_linked.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    return L


def model_linked(L, hist, block, R=512):
    """the LZ4 stream of `block` with the last <= 64 KiB of `hist` as its history"""
    hist = hist[-BLOCK:]
    buf = hist + block
    out = C.create_string_buffer(len(block) + len(block) // 255 + 32)
    n = L.enc2_model_lz4_linked(buf, len(hist), len(buf), out, R)
    assert n >= 0
    return out.raw[:n]


def block_seq(streams_and_blocks):
    """a frame's block sequence: size word + stream, or the block itself when the stream does not shrink it (LZ4F_makeBlock)"""
    out = bytearray()
    for c, blk in streams_and_blocks:
        if len(c) >= len(blk):
            out += struct.pack("<I", len(blk) | 0x80000000) + blk
        else:
            out += struct.pack("<I", len(c)) + c
    return bytes(out)


def linked_blocks(L, data, hist=b"", R=512):
    """what cj_lz4_frame_compress_blocks_linked writes through the batch kernel"""
    pairs = []
    for i in range(0, len(data), BLOCK):
        h = hist if i == 0 else data[i - BLOCK:i]
        blk = data[i:i + BLOCK]
        pairs.append((model_linked(L, h, blk, R), blk))
    return block_seq(pairs)


def independent_blocks(M, data, R=512):
    return block_seq([(model_lz4(M, data[i:i + BLOCK], R), data[i:i + BLOCK]) for i in range(0, len(data), BLOCK)])


def frame(blocks, data, flg):
    hdr = bytes([0x04, 0x22, 0x4D, 0x18, flg, 0x40])
    hdr += bytes([(oracle.xxh32(hdr[4:6]) >> 8) & 0xFF])
    return hdr + blocks + struct.pack("<II", 0, oracle.xxh32(data))


def corpus_streams(limit=4 << 20):
    """every corpus file larger than 64 KiB as one stream (its first 4 MiB; the sampled files as their chunks back to back)"""
    d = os.path.join(ROOT, "tests", "golden", "corpus")
    mf = json.load(open(os.path.join(d, "manifest.json")))
    for name in sorted(mf["files"]) + sorted(mf.get("samples", {})):
        raw = bz2.decompress(open(os.path.join(d, name + (".bz2" if name in mf["files"] else ".sample64k.bz2")), "rb").read())
        if len(raw) > BLOCK:
            yield name, raw[:limit]


def test_without_history_the_linked_model_is_the_independent_one():
    L, M = linked_lib(), model_lib()
    raws = [r for _, r in cases()] + [c for _, chunks in corpus_files() for c in chunks]
    for R in (256, 512):
        for raw in raws:
            assert model_linked(L, b"", raw, R) == model_lz4(M, raw, R), (R, len(raw))


def test_linked_frames_decode_with_the_oracle():
    L = linked_lib()
    streams = [("cases", b"".join(r for _, r in cases()))] + list(corpus_streams(1 << 20))
    for name, data in streams:
        f = frame(linked_blocks(L, data), data, 0x44)
        r, d = oracle.lz4_frame_decompress(f, len(data))
        assert r == len(data) and d == data, (name, r)
    # a block whose history is the tail of a previous flush (the streaming encoder): only the last 64 KiB of it count
    data = b"".join(r for _, r in cases())
    for cut in (1, 13, 4096, 65536, 65537, 200000):
        head, tail = data[:cut], data[cut:cut + 300000]
        f = frame(linked_blocks(L, head) + linked_blocks(L, tail, hist=head), head + tail, 0x44)
        r, d = oracle.lz4_frame_decompress(f, len(head) + len(tail))
        assert r == len(head) + len(tail) and d == head + tail, (cut, r)


def test_linking_saves_bytes_on_every_corpus_file_and_stays_near_liblz4():
    L, M = linked_lib(), model_lib()
    tot_i = tot_l = 0
    report = {}
    for name, data in corpus_streams():
        ind = len(independent_blocks(M, data))
        lnk = len(linked_blocks(L, data))
        ref = oracle.lz4_frame_compress(data, 4, 1)[0]          # liblz4's linked frame of 64 KiB blocks
        mine = lnk + 15
        report[name] = (len(data) / ind, len(data) / lnk, mine / ref)
        assert lnk <= ind, (name, ind, lnk)
        assert mine <= ref * 1.08, (name, mine, ref)
        tot_i += ind
        tot_l += lnk
    assert tot_l <= 0.97 * tot_i, (tot_l / tot_i, report)
