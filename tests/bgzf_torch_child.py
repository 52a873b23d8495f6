"""Child process of tests/test_bgzf_gpu.py: bgzf_compress_many_device on torch tensors on a side stream, then bgzf_sizes_device and
bgzf_decompress_many_device over what it wrote, with the encoder's device results as the decoder's in_len; then a batch of model
cases, malformed ones among them, through the device entries.  torch is imported BEFORE cramjam_amd, as a user of both has to
(tests/device_api_child.py says why)."""
import gzip
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bgzf_model as M  # noqa: E402
import device_batch as DB  # noqa: E402
import deflate_cases as D  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def round_trip(give_result):
    text = D.words(150000, 91)
    chunks = [text[:n] for n in (0, 1, 4000, 65280, 65281, 150000)]
    n = len(chunks)
    buf, off, ln = DB.pack(chunks, mis=0, dtype=np.int64)
    cap = np.array([batch.bgzf_compress_bound(int(x)) for x in ln], np.int64)
    ooff = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in, t_off, t_len = (torch.from_numpy(a).cuda() for a in (buf, off, ln))
        t_cap, t_ooff = torch.from_numpy(cap).cuda(), torch.from_numpy(ooff).cuda()
        t_out = torch.zeros(int(cap.sum()) + 64, dtype=torch.uint8, device="cuda")
        t_back = torch.zeros(buf.size, dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int64, device="cuda") if give_result else None
        res2 = torch.empty(n, dtype=torch.int64, device="cuda")
        res3 = torch.empty(n, dtype=torch.int64, device="cuda")
        got = batch.bgzf_compress_many_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, result=res, stream=side.cuda_stream, sync=False)
        clen = res if give_result else torch.from_numpy(np.asarray(got, np.int64)).cuda()
        assert not give_result or got is res
        batch.bgzf_sizes_device(t_out, t_ooff, clen, result=res3, stream=side.cuda_stream, sync=False)
        batch.bgzf_decompress_many_device(t_out, t_ooff, clen, t_back, t_off, t_len, result=res2, stream=side.cuda_stream, sync=False)
    side.synchronize()
    clen, res2, res3, out, back = clen.cpu().numpy(), res2.cpu().numpy(), res3.cpu().numpy(), t_out.cpu().numpy(), t_back.cpu().numpy()
    for i, c in enumerate(chunks):
        s = out[int(ooff[i]):int(ooff[i]) + int(clen[i])].tobytes()
        assert clen[i] > 0 and gzip.decompress(s) == c and M.decode(s) == (len(c), c), (i, clen[i])
        assert res2[i] == res3[i] == len(c) and back[int(off[i]):int(off[i]) + len(c)].tobytes() == c, (i, res2[i], res3[i])


def model_cases():
    names = [k for k in M.cases()][::3]
    streams = [M.cases()[k][1] for k in names]
    buf, off, ln = DB.pack(streams, mis=0, dtype=np.int64)
    sizes = np.array([M.sizes(s) for s in streams], np.int64)
    cap = np.maximum(sizes, 0)
    ooff = np.concatenate([[0], np.cumsum(cap + 16)[:-1]]).astype(np.int64)
    t_in = torch.from_numpy(buf).cuda()
    t_out = torch.zeros(int((cap + 16).sum()) + 64, dtype=torch.uint8, device="cuda")
    got_sizes = batch.bgzf_sizes_device(t_in, off, ln)
    assert list(got_sizes) == list(sizes)
    res = batch.bgzf_decompress_many_device(t_in, off, ln, t_out, ooff, cap)
    out = t_out.cpu().numpy()
    for i, k in enumerate(names):
        r, o = M.want(k)
        assert res[i] == r and (r < 0 or out[int(ooff[i]):int(ooff[i]) + r].tobytes() == o), (k, res[i], r)


if __name__ == "__main__":
    round_trip(True)
    round_trip(False)
    model_cases()
    print("bgzf torch: ok")
