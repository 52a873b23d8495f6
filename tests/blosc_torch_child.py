"""Child process of tests/test_blosc_gpu.py: Blosc chunk batches on torch tensors, on a side stream.  torch is imported BEFORE
cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import blosc_cases as K  # noqa: E402
import blosc_model as M  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def fixtures():
    vs = K.doc()["valid"]
    blob, off, ln = K.pack([v["bytes"] for v in vs])
    caps = np.array([v["nbytes"] for v in vs], np.uint64)
    ooff = np.concatenate([[0], np.cumsum((caps + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(blob).cuda()
        t = [torch.from_numpy(a.astype(np.int64)).cuda() for a in (off, ln, ooff, caps)]
        d_out = torch.zeros(int(ooff[-1] + caps[-1]) + 64, dtype=torch.uint8, device="cuda")
        res = torch.empty(len(vs), dtype=torch.int64, device="cuda")
        sz = torch.empty(len(vs), dtype=torch.int64, device="cuda")
        batch.blosc_chunk_sizes_device(d_in, t[0], t[1], result=sz, stream=side.cuda_stream, sync=False)
        batch.blosc_decompress_chunks_device(d_in, t[0], t[1], d_out, t[2], t[3], result=res, stream=side.cuda_stream)
    side.synchronize()
    res, sz, out = res.cpu().numpy(), sz.cpu().numpy(), d_out.cpu().numpy()
    for i, v in enumerate(vs):
        if v["supported"]:
            assert res[i] == v["nbytes"] == sz[i] and K.sha(out[int(ooff[i]):int(ooff[i]) + v["nbytes"]]) == v["sha256"], v["name"]
        else:
            assert res[i] == -31 and sz[i] == -31, v["name"]


def round_trip():
    n, S = 10000, 262144
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        base = torch.arange(n * S // 4, dtype=torch.float32, device="cuda") * 0.25
        raw = base.view(torch.uint8)
        off = torch.arange(n, dtype=torch.int64, device="cuda") * S
        ln = torch.full((n,), S, dtype=torch.int64, device="cuda")
        cstride = S + 32
        coff = torch.arange(n, dtype=torch.int64, device="cuda") * cstride
        ccap = torch.full((n,), cstride, dtype=torch.int64, device="cuda")
        comp = torch.empty(n * cstride + 64, dtype=torch.uint8, device="cuda")
        cres = torch.empty(n, dtype=torch.int64, device="cuda")
        batch.blosc_compress_chunks_device(raw, off, ln, comp, coff, ccap, 4, filter=1, result=cres, stream=side.cuda_stream)
        assert int(cres.min()) > 16 and int(cres.max()) < S // 2
        sz = torch.empty(n, dtype=torch.int64, device="cuda")
        batch.blosc_chunk_sizes_device(comp, coff, cres, result=sz, stream=side.cuda_stream, sync=False)
        back = torch.zeros(n * S, dtype=torch.uint8, device="cuda")
        dres = torch.empty(n, dtype=torch.int64, device="cuda")
        batch.blosc_decompress_chunks_device(comp, coff, cres, back, off, ln, result=dres, stream=side.cuda_stream)
        assert torch.equal(dres, sz) and torch.equal(dres, ln)
        assert torch.equal(back, raw)                                             # every byte, on the device
    side.synchronize()
    first = comp[:int(cres[0])].cpu().numpy().tobytes()
    assert M.decode(first) == raw[:S].cpu().numpy().tobytes()


if __name__ == "__main__":
    {"fixtures": fixtures, "round_trip": round_trip}[sys.argv[1]]()
    print(sys.argv[1] + ": ok")
