"""Child process of tests/test_frame_batch_gpu.py: torch is imported BEFORE cramjam_amd (see tests/device_api_child.py).  The device
calls of the frame batches on torch tensors, with and without a caller's stream, give the host batch's results and bytes."""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import device_batch as DB  # noqa: E402  (beside this script)
import cramjam_amd as cj  # noqa: E402
from cramjam_amd import _native as N  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def run(device_fn, host_fn, inputs, caps, stream):
    dev = torch.device("cuda:0")
    buf, off, ln = DB.pack(inputs, mis=lambda i: 5, gap=0)       # every input 5 bytes off a granule
    cap = np.array(caps, np.uint64)
    out_off = np.concatenate([[0], np.cumsum(cap + 16)[:-1]]).astype(np.uint64)
    t_in = torch.from_numpy(buf).to(dev)
    t_out = torch.full((int(out_off[-1] + cap[-1]) + 64,), 0xA5, dtype=torch.uint8, device=dev)
    t_off, t_len = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(ln.view(np.int64)).to(dev)
    t_ooff, t_cap = torch.from_numpy(out_off.view(np.int64)).to(dev), torch.from_numpy(cap.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    if stream:
        side = torch.cuda.Stream()
        t_res = torch.empty(len(inputs), dtype=torch.int64, device=dev)
        with torch.cuda.stream(side):
            device_fn(t_in, t_off, t_len, t_out, t_ooff, t_cap, result=t_res, stream=side.cuda_stream)
        side.synchronize()
        res = t_res.cpu().numpy().tolist()
    else:
        res = device_fn(t_in, off, ln, t_out, out_off, cap).tolist()
    host = t_out.cpu().numpy()
    hres, houts = host_fn(inputs, caps)
    assert res == list(hres), (res[:8], list(hres)[:8])
    for k in range(len(inputs)):
        if res[k] >= 0:
            assert bytes(host[int(out_off[k]):int(out_off[k]) + res[k]]) == bytes(houts[k]), k
        tail = host[int(out_off[k] + cap[k]):int(out_off[k] + cap[k]) + 16]
        assert (tail == 0xA5).all(), k
    return res


def main():
    r = random.Random(5)
    raws = [r.randbytes(n) if i % 2 else (b"frame batch " * (n // 12 + 1))[:n] for i, n in enumerate([0, 1, 777, 65536, 65537, 200000, 5000])]
    L = N.lib()
    for stream in (False, True):
        lz = [bytes(cj.lz4.compress(d)) for d in raws]
        lz[2] = lz[2][:-3]                                              # one truncated frame among them
        run(batch.lz4_decompress_frames_device, lambda f, c: batch.lz4_decompress_frames(f, output_lens=c), lz, [len(d) for d in raws], stream)
        sn = [bytes(cj.snappy.compress(d)) for d in raws]
        sn[3] = sn[3][:20]
        run(batch.snappy_decompress_framed_many_device, lambda f, c: batch.snappy_decompress_framed_many(f, output_lens=c), sn, [len(d) for d in raws], stream)
        run(batch.lz4_compress_frames_device, lambda d, c: batch.lz4_compress_frames(d), raws, [L.cj_lz4_frame_compress_bound(len(d)) for d in raws], stream)
        run(batch.snappy_compress_framed_many_device, lambda d, c: batch.snappy_compress_framed_many(d), raws,
            [L.cj_snappy_frame_max_compress_len(len(d)) for d in raws], stream)
    print("frame batch device: ok")


if __name__ == "__main__":
    main()
