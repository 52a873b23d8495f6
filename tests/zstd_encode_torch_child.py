"""Child process of tests/test_zstd_encode_gpu.py: zstd_compress_many_device on torch tensors, on a side stream, enqueue-only
(sync=False), then the decode of the same frames on that stream, compared after ONE synchronisation.  torch is imported BEFORE
cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import zstd_enc_cases as E  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def calls(checksum, give_result):
    keys = [k for k in E.cases() if len(E.cases()[k]) < 70000][::3]
    chunks = [E.cases()[k] for k in keys]
    n = len(chunks)
    ln = np.array([len(c) for c in chunks], np.int64)
    off = np.concatenate([[0], np.cumsum((ln + 31) & ~15)[:-1]]).astype(np.int64)
    buf = np.zeros(int(off[-1] + ln[-1]) + 64, np.uint8)
    for k, c in enumerate(chunks):
        buf[int(off[k]):int(off[k]) + len(c)] = np.frombuffer(c, np.uint8)
    cap = np.array([batch.zstd_compress_bound(int(x), checksum) for x in ln], np.int64)
    ooff = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in, t_off, t_len = (torch.from_numpy(a).cuda() for a in (buf, off, ln))
        t_cap, t_ooff = torch.from_numpy(cap).cuda(), torch.from_numpy(ooff).cuda()
        t_out = torch.zeros(int(cap.sum()) + 64, dtype=torch.uint8, device="cuda")
        t_back = torch.zeros(buf.size, dtype=torch.uint8, device="cuda")
        res = torch.empty(n, dtype=torch.int64, device="cuda") if give_result else None
        res2 = torch.empty(n, dtype=torch.int64, device="cuda")
        got = batch.zstd_compress_many_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, checksum=checksum, result=res, stream=side.cuda_stream, sync=False)
        if give_result:
            assert got is res
            clen = res            # the decoder reads the encoder's results where they are: nothing waits in between
        else:                     # (without a result tensor the call reads its results back, and so waits)
            clen = torch.from_numpy(np.asarray(got, np.int64)).cuda()
        batch.zstd_decompress_many_device(t_out, t_ooff, clen, t_back, t_off, t_len, result=res2, stream=side.cuda_stream, sync=False)
    side.synchronize()
    clen, res2, out, back = clen.cpu().numpy(), res2.cpu().numpy(), t_out.cpu().numpy(), t_back.cpu().numpy()
    for i, k in enumerate(keys):
        r, s = E.model(chunks[i], int(checksum))[:2]
        assert clen[i] == r and out[int(ooff[i]):int(ooff[i]) + r].tobytes() == s, (k, clen[i], r)
        assert res2[i] == len(chunks[i]) and back[int(off[i]):int(off[i]) + len(chunks[i])].tobytes() == chunks[i], (k, res2[i])


if __name__ == "__main__":
    calls(False, True)
    calls(True, False)
    print("zstd encode: ok")
