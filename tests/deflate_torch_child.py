"""Child process of tests/test_deflate_gpu.py: the device-resident DEFLATE calls on torch tensors, on a side stream, enqueue-only
(sync=False).  torch is imported BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import deflate_cases as D  # noqa: E402
import device_batch as DB  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def calls(wrap):
    cs = D.cases(wrap)
    name = D.WRAP_NAME[wrap]
    buf, off, ln = DB.pack([c["bytes"] for c in cs], mis=0, dtype=np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in = torch.from_numpy(buf).cuda()
        t_off, t_len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
        n = len(cs)
        sz, res = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
        # the two-call pattern: sizes (enqueue only), capacities computed on the device, decode (enqueue only) — all on the caller's stream
        batch.deflate_sizes_device(t_in, t_off, t_len, wrapper=name, result=sz, stream=side.cuda_stream, sync=False)
        cap = sz.clamp(min=0)
        ooff = cap.cumsum(0) - cap
        t_out = torch.zeros(int(cap.sum()) + 64, dtype=torch.uint8, device="cuda")
        batch.deflate_decompress_many_device(t_in, t_off, t_len, t_out, ooff, cap, wrapper=name, result=res, stream=side.cuda_stream, sync=False)
        out, ooff = t_out.cpu().numpy(), ooff.cpu().numpy()           # (ordered behind the decode on the side stream)
    side.synchronize()
    sz, res = sz.cpu().numpy(), res.cpu().numpy()
    for i, c in enumerate(cs):
        want = D.size_verdict(wrap, c["bytes"])
        assert sz[i] == want, (c["name"], sz[i], want)
        if want < 0:
            continue
        r, raw = D.verdict(wrap, c["bytes"], want)
        assert res[i] == r and (r < 0 or out[int(ooff[i]):int(ooff[i]) + r].tobytes() == raw), (c["name"], res[i], r)


if __name__ == "__main__":
    for w in D.WRAPS:
        calls(w)
    print("deflate: ok")
