"""Child process of tests/test_parquet_write_gpu.py: Parquet-to-Parquet recompression on torch tensors without leaving a side stream —
parquet_decompress_chunks_device, parquet_pages_device and parquet_compress_chunks_device one behind the other, device-resident
metadata, result tensors, sync=False: the decoder's output and the pages query's table are the writer's input as they lie —, then the
writer with host metadata.  The written chunks are the host batch's, byte for byte, and decode to the golden bytes.  torch is imported
BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import parquet_model as M  # noqa: E402
import device_batch as DB  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def golden_inputs(src):
    gs = M.golden_of(src, big=False)
    buf, off, ln = DB.pack([g["chunk"] for g in gs], mis=0, dtype=np.int64)
    sizes = np.array([g["decoded_len"] for g in gs], np.int64)
    counts = np.array([len(g["pages"]) for g in gs], np.int64)
    return gs, buf, off, ln, sizes, counts


def host_written(gs, dst):
    """what the host batch writes for the same decoded chunks and tables (num_nulls stays 0, as the pages query leaves it)"""
    res, chunks = batch.parquet_compress_chunks([M.plain_of(g) for g in gs], [g["pages"] for g in gs], dst)
    assert all(r > 0 for r in res)
    return [bytes(c) for c in chunks]


def on_a_side_stream(src, dst):
    gs, buf, off, ln, sizes, counts = golden_inputs(src)
    n = len(gs)
    caps = np.array([batch.parquet_compress_bound(dst, int(s), int(c)) for s, c in zip(sizes, counts)], np.int64)
    slots = (caps + 15) // 16 * 16
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in, t_off, t_len, t_size, t_count, t_cap = (torch.from_numpy(a).cuda() for a in (buf, off, ln, sizes, counts, caps))
        t_ooff = torch.from_numpy(np.cumsum(sizes + 16) - (sizes + 16)).cuda()
        t_roff = torch.cumsum(t_count, 0) - t_count
        t_woff = torch.from_numpy(np.cumsum(slots) - slots).cuda()
        t_dec = torch.zeros(int((sizes + 16).sum()) + 64, dtype=torch.uint8, device="cuda")
        t_rows = torch.zeros(8 * int(counts.sum()) + 8, dtype=torch.int64, device="cuda")
        t_out = torch.full((int(slots.sum()) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        r_dec, r_pages, r_enc = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3))
        batch.parquet_decompress_chunks_device(t_in, t_off, t_len, t_dec, t_ooff, t_size, src, result=r_dec, stream=side.cuda_stream, sync=False)
        batch.parquet_pages_device(t_in, t_off, t_len, rows=t_rows, row_off=t_roff, row_cap=t_count, result=r_pages, stream=side.cuda_stream, sync=False)
        got = batch.parquet_compress_chunks_device(t_dec, t_ooff, t_size, t_rows, t_roff, t_count, t_out, t_woff, t_cap, dst, result=r_enc,
                                                   stream=side.cuda_stream, sync=False)
        assert got is r_enc
    side.synchronize()
    assert r_dec.cpu().tolist() == list(sizes) and r_pages.cpu().tolist() == list(counts)
    out, res, woff = t_out.cpu().numpy(), r_enc.cpu().tolist(), (np.cumsum(slots) - slots)
    want = host_written(gs, dst)
    for i, g in enumerate(gs):
        assert res[i] == len(want[i]) and out[int(woff[i]):int(woff[i]) + res[i]].tobytes() == want[i], (src, dst, g["name"], res[i])
        assert (out[int(woff[i]) + res[i]:int(woff[i]) + int(slots[i])] == 0xA5).all(), (src, dst, g["name"])
    back, outs = batch.parquet_decompress_chunks(want, dst, output_lens=[int(s) for s in sizes], verify_crc=True)
    assert list(back) == list(sizes) and [M.digest(o) for o in outs] == [g["sha256"] for g in gs], (src, dst)


def with_host_metadata(src, dst):
    gs = M.golden_of(src, 2, big=False)
    plain = [M.plain_of(g) for g in gs]
    buf, off, ln = DB.pack(plain, mis=0, dtype=np.int64)
    rows = np.array([r for g in gs for r in g["pages"]], np.int64).reshape(-1)
    counts = np.array([len(g["pages"]) for g in gs], np.int64)
    caps = np.array([batch.parquet_compress_bound(dst, len(p), int(c)) for p, c in zip(plain, counts)], np.int64)
    woff = np.cumsum(caps + 16) - (caps + 16)
    t_in, t_rows = torch.from_numpy(buf).cuda(), torch.from_numpy(rows).cuda()
    t_out = torch.zeros(int((caps + 16).sum()) + 64, dtype=torch.uint8, device="cuda")
    res = batch.parquet_compress_chunks_device(t_in, off, ln, t_rows, np.cumsum(counts) - counts, counts, t_out, woff, caps, dst)
    out, want = t_out.cpu().numpy(), host_written(gs, dst)
    for i, g in enumerate(gs):
        assert res[i] == len(want[i]) and out[int(woff[i]):int(woff[i]) + int(res[i])].tobytes() == want[i], (src, dst, g["name"], res[i])


if __name__ == "__main__":
    names = list(M.CODECS)
    for k, src in enumerate(names):
        dst = names[(k + 2) % len(names)]
        on_a_side_stream(src, dst)
        with_host_metadata(dst, src)
    print("parquet write torch: ok")
