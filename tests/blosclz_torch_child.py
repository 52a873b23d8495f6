"""Child process of tests/test_blosclz_gpu.py: the device-resident Blosc calls with blosclz=True on torch tensors, on a side stream.
torch is imported BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import blosc_cases as K  # noqa: E402
import blosclz_model as Z  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def fixtures():
    vs = Z.valid()
    blob, off, ln = K.pack([v["bytes"] for v in vs])
    caps = np.array([v["nbytes"] for v in vs], np.uint64)
    ooff = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(blob).cuda()
        t = [torch.from_numpy(a.astype(np.int64)).cuda() for a in (off, ln, ooff, caps)]
        d_out = torch.zeros(int(ooff[-1] + caps[-1]) + 64, dtype=torch.uint8, device="cuda")
        res, sz, res0, sz0 = (torch.empty(len(vs), dtype=torch.int64, device="cuda") for _ in range(4))
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz, stream=side.cuda_stream, sync=False, blosclz=True)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res, stream=side.cuda_stream, blosclz=True)
        out = d_out.cpu().numpy()
        # the default reading on the same tensors: refused, as before
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz0, stream=side.cuda_stream, sync=False)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res0, stream=side.cuda_stream)
    side.synchronize()
    res, sz, res0, sz0 = (x.cpu().numpy() for x in (res, sz, res0, sz0))
    for i, v in enumerate(vs):
        assert res[i] == v["nbytes"] == sz[i] and Z.sha(out[int(ooff[i]):int(ooff[i]) + v["nbytes"]]) == v["sha256"], v["name"]
        want = -31 if Z.is_blosclz(v["bytes"]) else v["nbytes"]
        assert res0[i] == want and sz0[i] == want, v["name"]
    assert (out[int(ooff[-1] + caps[-1]):] == 0).all()


if __name__ == "__main__":
    fixtures()
    print("fixtures: ok")
