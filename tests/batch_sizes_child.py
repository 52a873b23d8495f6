"""Child process of tests/test_batch_sizes_gpu.py: the decoded-size queries on the GPU, from torch tensors.  torch is imported BEFORE
cramjam_amd, as a user of both has to (tests/device_api_child.py says why).  Every figure a check compares is printed before it asserts."""
import bz2
import ctypes as C
import json
import os
import sys
import time
from base64 import b64decode

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import batch_sizes_cases as K  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A5A5A5A5A


def pack_odd(blobs):
    """every chunk at an odd byte offset, a few bytes apart"""
    off, run = [], 1
    for k, b in enumerate(blobs):
        off.append(run)
        run += len(b) + (k % 5)
        run |= 1
    buf = np.full(run + 64, 0xEE, np.uint8)
    for o, b in zip(off, blobs):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return buf, np.array(off, np.uint64), np.array([len(b) for b in blobs], np.uint64)


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def query(fn, blobs, stream=None, **kw):
    """fn over one device batch of blobs at odd offsets; checks the guard words around result and the input buffer"""
    buf, off, ln = pack_odd(blobs)
    n = len(blobs)
    t_in, t_off, t_len = torch.from_numpy(buf).to(DEV), dev_i64(off), dev_i64(ln)
    t_all = torch.full((n + 16,), GUARD, dtype=torch.int64, device=DEV)
    t_res = t_all[8:8 + n]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = fn(t_in, t_off, t_len, result=t_res, stream=side.cuda_stream, sync=False, **kw)
    assert r is t_res
    side.synchronize()
    got = t_all.cpu().numpy()
    assert (got[:8] == GUARD).all() and (got[8 + n:] == GUARD).all(), "guard words around result were written"
    assert (t_in.cpu().numpy() == buf).all(), "the input buffer was written"
    return [int(x) for x in got[8:8 + n]]


def corpus_chunks():
    out = []
    d = os.path.join(K.GOLDEN, "corpus")
    for f in sorted(os.listdir(d)):
        if f.endswith(".bz2"):
            raw = bz2.decompress(open(os.path.join(d, f), "rb").read())
            out += [raw[i:i + 65536] for i in range(0, len(raw), 65536)]
    return out


_expect = {}


def expect(blob):
    if blob not in _expect:
        _expect[blob] = K.expected_size(blob)
    return _expect[blob]


def raw_lz4_cases():
    cases = K.lz4_cases()
    cases += [(("corpus", i), oracle.lz4_compress_raw(c)[1], True) for i, c in enumerate(corpus_chunks())]
    for n in (1, 65535, 65536, 65537, 256 << 10):
        cases.append((("text", n), oracle.lz4_compress_raw(K.text(n, n))[1], True))
        cases.append((("random", n), oracle.lz4_compress_raw(np.random.default_rng(n).integers(0, 256, n, np.uint8).tobytes())[1], True))
    cases += [(("empty", i), b"", False) for i in range(3)]
    return cases


def test_raw_lz4_sizes_equal_the_oracle(cases):
    blobs = [b for _, b, _ in cases]
    want = [expect(b) for b in blobs]
    got = query(batch.lz4_block_sizes_device, blobs)
    bad = [(cases[i][0], len(blobs[i]), got[i], want[i]) for i in range(len(blobs)) if got[i] != want[i]]
    print("raw lz4: %d chunks, %d accepted, %d above the lane limit, mismatches %d" % (len(blobs), sum(w >= 0 for w in want), sum(len(b) > 65824 for b in blobs), len(bad)), flush=True)
    assert not bad, bad[:10]
    # the same chunks as batches of 1, 63, 64, 65 (one of them above 64 KiB) and tiled to 24 576
    order = sorted(range(len(blobs)), key=lambda i: (i * 7919) % len(blobs))
    for n in (1, 63, 64, 65):
        idx = order[:n - 1] + [next(i for i in order if len(blobs[i]) > 100000)]
        g = query(batch.lz4_block_sizes_device, [blobs[i] for i in idx])
        print("raw lz4: n = %d: %s" % (n, g == [want[i] for i in idx]), flush=True)
        assert g == [want[i] for i in idx], n
    small = [i for i in order if len(blobs[i]) < 200000]
    idx = [small[k % len(small)] for k in range(24576)]
    g = query(batch.lz4_block_sizes_device, [blobs[i] for i in idx])
    print("raw lz4: n = 24576: %s" % (g == [want[i] for i in idx]), flush=True)
    assert g == [want[i] for i in idx]


def test_contract_with_the_decoder(cases):
    """sizes -> decode on ONE side stream, the query with sync=False, capacities computed on the device, one synchronisation"""
    ours = batch.lz4_compress_blocks([K.text(50000, 5), oracle.synth_v1(65536, 77), b"x" * 3000, K.text(200000, 6)], store_size=False)[1]
    cases = cases + [(("ours", i), bytes(b), True) for i, b in enumerate(ours)]
    for slack, pick in ((K.SLACK, lambda c: expect(c[1]) >= 0), (0, lambda c: c[2] and expect(c[1]) >= 0)):
        sel = [c for c in cases if pick(c)]
        blobs = [b for _, b, _ in sel]
        S = [expect(b) for b in blobs]
        buf, off, ln = pack_odd(blobs)
        n = len(blobs)
        t_in, t_off, t_len = torch.from_numpy(buf).to(DEV), dev_i64(off), dev_i64(ln)
        t_size = torch.empty(n, dtype=torch.int64, device=DEV)
        t_res = torch.empty(n, dtype=torch.int64, device=DEV)
        t_out = torch.full((sum(S) + (slack + 16) * n + 64,), 0xAB, dtype=torch.uint8, device=DEV)       # (sized from the oracle: no read-back here)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            batch.lz4_block_sizes_device(t_in, t_off, t_len, result=t_size, stream=side.cuda_stream, sync=False)
            cap = t_size.clamp(min=0) + slack
            pitch = cap + 16
            o_off = pitch.cumsum(0) - pitch
            batch.lz4_decompress_blocks_device(t_in, t_off, t_len, t_out, o_off, cap, result=t_res, stream=side.cuda_stream, sync=False)
        side.synchronize()
        res, oo, out = t_res.cpu().numpy(), o_off.cpu().numpy(), t_out.cpu().numpy()
        bad = [(sel[i][0], int(res[i]), S[i]) for i in range(n) if res[i] != S[i]]
        print("contract: cap = S + %d: %d chunks, wrong results %d" % (slack, n, len(bad)), flush=True)
        assert not bad, bad[:10]
        for i in range(n):
            assert out[int(oo[i]):int(oo[i]) + S[i]].tobytes() == oracle.lz4_decompress_raw(blobs[i], S[i] + K.SLACK)[1], sel[i][0]


def lz4_frame(bd, blocks, flg=0x60):
    """a hand-made frame: no checksums, no content size; blocks = [(word, payload)]"""
    desc = bytes([flg, bd])
    out = bytearray((0x184D2204).to_bytes(4, "little") + desc + bytes([(oracle.xxh32(desc) >> 8) & 0xff]))
    for w, p in blocks:
        out += w.to_bytes(4, "little") + p
    return bytes(out + bytes(4))


def test_header_and_frame_queries():
    L = N.lib()
    g = json.load(open(os.path.join(K.GOLDEN, "golden_vectors.json")))

    def host(fn, b):
        a = np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8)
        return int(fn(a.ctypes.data, len(b)))
    # Snappy raw
    sn = [b64decode(v["snappy"]) for v in g["vectors"]] + [b64decode(m["data"]) for m in g["malformed_snappy"]]
    sn += [b"", b"\x80", b"\xff\xff\xff\xff\x0f", b"\xff\xff\xff\xff\x1f", b"\x80" * 12, b"\x00", b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\x02"]
    got = query(batch.snappy_raw_sizes_device, sn)
    print("snappy raw: %d chunks, %d errors" % (len(sn), sum(x < 0 for x in got)), flush=True)
    for b, x in zip(sn, got):
        assert x == host(L.cj_snappy_raw_decompress_len, b) and (x == oracle.snappy_decompress_len(b) if len(b) else x == 0), (b[:12], x)
    # prefixed LZ4
    pre = [len(b64decode(v["raw"])).to_bytes(4, "little") + b64decode(v["lz4"]) for v in g["vectors"] if "raw" in v]
    want = [host(L.cj_lz4_block_prefixed_len, b) for b in pre]
    pre += [b"", b"\x01", b"abc", b"\xff\xff\xff\xff", b"\x00\x00\x00\x80rest", b"\x01\x00\x00\x7e", b"\x00\x00\x00\x7e", b"\x00\x00\x00\x00"]
    want += [-3, -3, -3, -4, -4, -5, 0x7E000000, 0]
    got = query(batch.lz4_block_sizes_device, pre, store_size=True)
    print("prefixed lz4: %d chunks: %s" % (len(pre), got == want), flush=True)
    assert got == want, [(g_, w) for g_, w in zip(got, want) if g_ != w][:10]
    # LZ4 frames
    f = json.load(open(os.path.join(K.GOLDEN, "golden_frames.json")))
    frames = [b64decode(v["frame"]) for v in f["vectors"]] + [open(os.path.join(K.GOLDEN, "plaintext.txt.lz4"), "rb").read()]
    whole = frames[0]
    frames += [b"", (0x184D2A51).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"hello",
               whole[:len(whole) // 2], whole[:6], whole[:9], b"\x05" + whole[1:], whole[:4] + b"\xe4" + whole[5:], whole + b"trailing",
               lz4_frame(0x70, [(0x80000001, bytes([i & 255])) for i in range(3000)]),
               lz4_frame(0x70, [(0x80000001, b"a")] * 2000 + [(len(K.huge_match_block()[:40]), K.huge_match_block()[:40])] + [(0x80000001, b"b")] * 2000),
               lz4_frame(0x30, [(1, b"\x00")])]
    got = query(batch.lz4_frame_bounds_device, frames)
    print("lz4 frames: %d frames, %d errors" % (len(frames), sum(x < 0 for x in got)), flush=True)
    for b, x in zip(frames, got):
        assert x == host(L.cj_lz4_frame_decompress_bound, b) == oracle.lz4_frame_decompress_bound(b), (len(b), x, host(L.cj_lz4_frame_decompress_bound, b), oracle.lz4_frame_decompress_bound(b))
    assert got[len(f["vectors"]) + 1 + 8] == 3000
    # Snappy framed streams
    raws = [K.text(n, n) for n in (0, 1, 100, 65536, 65537, 300000)] + [np.random.default_rng(3).integers(0, 256, 150000, np.uint8).tobytes()]
    streams = [oracle.snappy_frame_compress(r)[1] for r in raws] + [open(os.path.join(K.GOLDEN, "plaintext.txt.snappy"), "rb").read()]
    s0 = streams[5]
    streams += [s0[:len(s0) // 2], s0[:3], s0[:10], b"\x00" + s0[1:], s0[:10] + b"\x02\x05\x00\x00hello", s0 + b"\xfe\x03\x00\x00pad", s0 + s0, b"\xff\x06\x00\x00sNaPpX"]
    got = query(batch.snappy_framed_sizes_device, streams)
    print("snappy framed: %d streams, %d errors" % (len(streams), sum(x < 0 for x in got)), flush=True)
    for b, x in zip(streams, got):
        assert x == host(L.cj_snappy_frame_decompress_len, b) == oracle.snappy_frame_decompress_len(b), (len(b), x)


def test_host_variants_and_decode_without_lengths(cases):
    sel = [c for c in cases if len(c[1]) < (1 << 20)]
    blobs = [b for _, b, _ in sel]
    want = [expect(b) for b in blobs]
    saved = dict(batch._engines)
    try:
        batch._engines.clear()
        batch._engines[0] = N.Engine(0)
        batch._engines["second"] = N.Engine(0)
        for devs in ([0], [0, "second"]):
            assert batch.lz4_block_sizes(blobs, devices=devs) == want, devs
            res, outs = batch.lz4_decompress_blocks(blobs, devices=devs)
            ok = [i for i, w in enumerate(want) if w >= 0]
            res2, outs2 = batch.lz4_decompress_blocks([blobs[i] for i in ok], [want[i] for i in ok], devices=devs)
            # (capacity S: a damaged block the query accepts may still ask the decoder for up to 12 bytes more — the same verdict either way)
            assert [res[i] for i in ok] == list(res2) and [bytes(outs[i]) for i in ok] == [bytes(o) for o in outs2]
            assert all(res[i] == want[i] for i in range(len(want)) if sel[i][2] or want[i] < 0), [(sel[i][0], res[i], want[i]) for i in range(len(want)) if res[i] != want[i]][:10]
            assert all(bytes(outs[i]) == oracle.lz4_decompress_raw(blobs[i], want[i])[1] for i in ok if sel[i][2])
            assert all(len(outs[i]) == 0 for i, w in enumerate(want) if w < 0)
            print("host: devices %s: %d blocks, %d rejected with their code and an empty output" % (devs, len(blobs), sum(w < 0 for w in want)), flush=True)
        pre = [len(r).to_bytes(4, "little") + oracle.lz4_compress_raw(r)[1] for r in (K.text(1000, 1), b"", K.text(70000, 2))] + [b"ab"]
        assert batch.lz4_block_sizes(pre, store_size=True) == [1000, 0, 70000, -3]
        res, outs = batch.lz4_decompress_blocks(pre, store_size=True)
        assert list(res) == [1000, 0, 70000, -3] and bytes(outs[2]) == K.text(70000, 2) and len(outs[3]) == 0
        sn = [oracle.snappy_compress(K.text(5000, 9))[1], b"", b"\x80"]
        assert batch.snappy_raw_sizes(sn, devices=[0, "second"]) == [5000, 0, oracle.snappy_decompress_len(b"\x80")]
        fr = [oracle.lz4_frame_compress(K.text(100000, 4), 4, oracle.LZ4F_CONTENT_SIZE)[1], b"junk junk"]
        assert batch.lz4_frame_bounds(fr) == [100000, oracle.lz4_frame_decompress_bound(fr[1])]
        st = [oracle.snappy_frame_compress(K.text(100000, 4))[1], b"junk junk"]
        assert batch.snappy_framed_sizes(st, devices=[0, "second"]) == [100000, oracle.snappy_frame_decompress_len(st[1])]
    finally:
        for k in (0, "second"):
            e = batch._engines.pop(k, None)
            if e is not None:
                e.close()
        batch._engines.clear()
        batch._engines.update(saved)


def test_a_frame_query_does_not_wait_for_a_queued_frame_batch():
    """tests/test_big_chunks_gpu.py's pattern ("the sixth submit returns while they run") and its bound: the query's call returns in
    less than half the time the queued frame batches take to drain"""
    raw = K.text(4 << 20, 8)
    frame = oracle.lz4_frame_compress(raw, 4, oracle.LZ4F_LINKED)[1]             # linked blocks: one wavefront chain per frame, slow on purpose
    n = 64
    buf, off, ln = pack_odd([frame] * n)
    t_in, t_off, t_len = torch.from_numpy(buf).to(DEV), dev_i64(off), dev_i64(ln)
    cap = np.full(n, len(raw), np.uint64)
    t_cap, t_ooff = dev_i64(cap), dev_i64(np.arange(n, dtype=np.uint64) * np.uint64(len(raw) + 64))
    t_out = torch.empty(n * (len(raw) + 64), dtype=torch.uint8, device=DEV)
    t_res, t_q = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    batch.lz4_decompress_frames_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, result=t_res, stream=a.cuda_stream)       # warm: scratch, code objects
    batch.lz4_frame_bounds_device(t_in, t_off, t_len, result=t_q, stream=b.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        batch.lz4_decompress_frames_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, result=t_res, stream=a.cuda_stream, sync=False)
    t1 = time.perf_counter()
    batch.lz4_frame_bounds_device(t_in, t_off, t_len, result=t_q, stream=b.cuda_stream, sync=False)
    asked = time.perf_counter() - t1
    b.synchronize()
    answered = time.perf_counter() - t1
    a.synchronize()
    drained = time.perf_counter() - t1
    print("frame query next to queued frame batches: call %.6f s, answer %.6f s, batches drained after %.6f s (queued in %.6f s)" % (asked, answered, drained, t1 - t0), flush=True)
    assert (t_res.cpu().numpy() == len(raw)).all() and (t_q.cpu().numpy() == oracle.lz4_frame_decompress_bound(frame)).all()
    assert asked < 0.5 * drained, (asked, drained)


if __name__ == "__main__":
    cases = raw_lz4_cases()
    test_raw_lz4_sizes_equal_the_oracle(cases)
    test_contract_with_the_decoder(cases)
    test_header_and_frame_queries()
    test_host_variants_and_decode_without_lengths(cases)
    test_a_frame_query_does_not_wait_for_a_queued_frame_batch()
    print("batch sizes: ok")
