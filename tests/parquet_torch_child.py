"""Child process of tests/test_parquet_gpu.py: parquet_chunk_sizes_device, parquet_pages_device and parquet_decompress_chunks_device on
torch tensors on a side stream — the two queries enqueue-only, with device-resident metadata, result tensors and sync=False; the pages
query's counts lay out its own table without leaving the stream —, then the same entries with host metadata.  torch is imported BEFORE
cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
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


def on_a_side_stream(codec, verify):
    gs = M.golden_of(codec)
    n = len(gs)
    buf, off, ln = DB.pack([g["chunk"] for g in gs], mis=0, dtype=np.int64)
    sizes = np.array([g["decoded_len"] for g in gs], np.int64)
    counts = np.array([len(g["pages"]) for g in gs], np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in, t_off, t_len = (torch.from_numpy(a).cuda() for a in (buf, off, ln))
        r_size, r_count, r_pages, r_dec = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(4))
        assert batch.parquet_chunk_sizes_device(t_in, t_off, t_len, codec, result=r_size, stream=side.cuda_stream, sync=False) is r_size
        assert batch.parquet_pages_device(t_in, t_off, t_len, result=r_count, stream=side.cuda_stream, sync=False) is r_count
        # the answers stay on the device: the sizes are the capacities, their running sums the offsets, of the decode and of the table
        t_ooff = torch.cumsum(r_size, 0) - r_size
        t_roff = torch.cumsum(r_count, 0) - r_count
        t_out = torch.zeros(int(sizes.sum()) + 64, dtype=torch.uint8, device="cuda")
        t_rows = torch.zeros(8 * int(counts.sum()) + 8, dtype=torch.int64, device="cuda")
        batch.parquet_pages_device(t_in, t_off, t_len, rows=t_rows, row_off=t_roff, row_cap=r_count, result=r_pages, stream=side.cuda_stream, sync=False)
        batch.parquet_decompress_chunks_device(t_in, t_off, t_len, t_out, t_ooff, r_size, codec, verify_crc=verify, result=r_dec, stream=side.cuda_stream, sync=False)
    side.synchronize()
    assert r_size.cpu().tolist() == r_dec.cpu().tolist() == list(sizes) and r_count.cpu().tolist() == r_pages.cpu().tolist() == list(counts), codec
    out, rows = t_out.cpu().numpy(), t_rows.cpu().numpy()
    p = r = 0
    for g in gs:
        assert M.digest(out[p:p + g["decoded_len"]]) == g["sha256"], (codec, g["name"])
        assert rows[8 * r:8 * (r + len(g["pages"]))].reshape(-1, 8).tolist() == g["pages"], (codec, g["name"])
        p += g["decoded_len"]; r += len(g["pages"])


def with_host_metadata(codec):
    gs = M.golden_of(codec, 2)
    buf, off, ln = DB.pack([g["chunk"] for g in gs], mis=0, dtype=np.int64)
    sizes = np.array([g["decoded_len"] for g in gs], np.int64)
    ooff = np.concatenate([[0], np.cumsum(sizes + 16)[:-1]]).astype(np.int64)
    t_in = torch.from_numpy(buf).cuda()
    t_out = torch.zeros(int((sizes + 16).sum()) + 64, dtype=torch.uint8, device="cuda")
    assert list(batch.parquet_chunk_sizes_device(t_in, off, ln, codec)) == list(sizes)
    assert list(batch.parquet_pages_device(t_in, off, ln)) == [len(g["pages"]) for g in gs]
    res = batch.parquet_decompress_chunks_device(t_in, off, ln, t_out, ooff, sizes, codec, verify_crc=True)
    out = t_out.cpu().numpy()
    for i, g in enumerate(gs):
        assert res[i] == sizes[i] and M.digest(out[int(ooff[i]):int(ooff[i]) + int(sizes[i])]) == g["sha256"], (codec, g["name"], res[i])


if __name__ == "__main__":
    for k, codec in enumerate(M.CODECS):
        on_a_side_stream(codec, k % 2 == 0)
        with_host_metadata(codec)
    print("parquet torch: ok")
