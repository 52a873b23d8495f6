"""Child process of tests/test_zstd_gpu.py: the device-resident Zstandard calls on torch tensors, on a side stream, enqueue-only
(sync=False): the 300 000-byte three-block frame and the 150 000-byte Treeless frame at three input alignments — the size query, the
capacities computed on the device, the decode, one synchronise.  torch is imported BEFORE cramjam_amd (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import zstd_cases as Z  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def main():
    by = {c.name: c for c in Z.load_cases()}
    picked = [by["mixed_300k"], by["text_150k_l1"], by["hand_cross_block"]]
    assert "lit:treeless" in by["text_150k_l1"].tags
    cs, off, run = [], [], 0
    for mis in (0, 1, 3):
        for c in picked:
            cs.append(c)
            off.append(run + mis)
            run += (mis + len(c.stream) + 15) // 16 * 16 + 16
    buf = np.zeros(run + 64, np.uint8)
    for o, c in zip(off, cs):
        buf[o:o + len(c.stream)] = np.frombuffer(c.stream, np.uint8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_in = torch.from_numpy(buf).cuda()
        t_off = torch.tensor(off, dtype=torch.int64).cuda()
        t_len = torch.tensor([len(c.stream) for c in cs], dtype=torch.int64).cuda()
        n = len(cs)
        sz, res = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
        batch.zstd_sizes_device(t_in, t_off, t_len, result=sz, stream=side.cuda_stream, sync=False)
        cap = sz.clamp(min=0)                                      # nothing copied back in between
        ooff = cap.cumsum(0) - cap
        t_out = torch.zeros(sum(c.cap for c in cs) + 64, dtype=torch.uint8, device="cuda")
        batch.zstd_decompress_many_device(t_in, t_off, t_len, t_out, ooff, cap, result=res, stream=side.cuda_stream, sync=False)
    side.synchronize()
    out, ooff, sz, res = t_out.cpu().numpy(), ooff.cpu().numpy(), sz.cpu().numpy(), res.cpu().numpy()
    for i, c in enumerate(cs):
        assert sz[i] == res[i] == c.verdicts[0], (c.name, sz[i], res[i])
        assert Z.sha(out[int(ooff[i]):int(ooff[i]) + int(res[i])]) == c.sha, c.name
    print("zstd: ok")


if __name__ == "__main__":
    main()
