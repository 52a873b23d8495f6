"""Child process of tests/test_blosc_zcodecs_gpu.py: the device-resident Blosc calls with zlib=True, zstd=True on torch tensors, on a
side stream.  torch is imported BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why).  Fixtures only: the
recorded sha256, no model, no libzstd."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import blosc_cases as K  # noqa: E402
import blosc_zcodec_model as Z  # noqa: E402
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
        res, sz, res0, sz0, res8, sz8 = (torch.empty(len(vs), dtype=torch.int64, device="cuda") for _ in range(6))
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz, stream=side.cuda_stream, sync=False, zlib=True, zstd=True)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res, stream=side.cuda_stream, zlib=True, zstd=True)
        out = d_out.cpu().numpy()
        # the default reading on the same tensors: refused, as before; with zlib=True alone the Zstd chunks are
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz0, stream=side.cuda_stream, sync=False)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res0, stream=side.cuda_stream)
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz8, stream=side.cuda_stream, sync=False, zlib=True)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res8, stream=side.cuda_stream, zlib=True)
    side.synchronize()
    res, sz, res0, sz0, res8, sz8 = (x.cpu().numpy() for x in (res, sz, res0, sz0, res8, sz8))
    for i, v in enumerate(vs):
        assert res[i] == v["nbytes"] == sz[i] and Z.sha(out[int(ooff[i]):int(ooff[i]) + v["nbytes"]]) == v["sha256"], v["name"]
        f = Z.fmt_of(v["bytes"])
        want = -31 if f is not None else v["nbytes"]
        assert res0[i] == want and sz0[i] == want, v["name"]
        want = -31 if f == Z.FORMAT_ZSTD else v["nbytes"]
        assert res8[i] == want and sz8[i] == want, v["name"]
    assert (out[int(ooff[-1] + caps[-1]):] == 0).all()


if __name__ == "__main__":
    fixtures()
    print("fixtures: ok")
