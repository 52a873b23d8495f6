"""Child process of tests/test_lz4_dict_gpu.py: the device-resident LZ4 block calls with dictionary=<tensor> on torch tensors, on a
side stream.  torch is imported BEFORE cramjam_amd, as a user of both has to (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import device_batch as DB  # noqa: E402
import lz4_dict_model as D  # noqa: E402
from cramjam_amd import batch  # noqa: E402


def dictionary_calls():
    dl = 65536
    cs = D.cases(dl)
    buf, off, ln = DB.pack([c["bytes"] for c in cs], mis=0, dtype=np.int64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_dict = torch.from_numpy(np.frombuffer(D.dictionary(dl), np.uint8).copy()).cuda()
        t_in = torch.from_numpy(buf).cuda()
        t_off, t_len = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
        n = len(cs)
        sz, res = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
        # the two-call pattern: sizes (enqueue only), capacities computed on the device, decode — all on the caller's stream
        batch.lz4_block_sizes_device(t_in, t_off, t_len, result=sz, stream=side.cuda_stream, sync=False, dictionary=t_dict)
        cap = sz.clamp(min=0) + batch.LZ4_SIZE_SLACK
        ooff = cap.cumsum(0) - cap
        t_out = torch.zeros(int(cap.sum()) + 64, dtype=torch.uint8, device="cuda")
        batch.lz4_decompress_blocks_device(t_in, t_off, t_len, t_out, ooff, cap, result=res, stream=side.cuda_stream, dictionary=t_dict)
        out, ooff = t_out.cpu().numpy(), ooff.cpu().numpy()
    side.synchronize()
    sz, res = sz.cpu().numpy(), res.cpu().numpy()
    d = D.dictionary(dl)
    for i, c in enumerate(cs):
        assert sz[i] == D.size_walk(c["bytes"], dl), c["name"]
        if sz[i] < 0:
            assert res[i] == D.CORRUPT, c["name"]                     # (with room that never runs out the decoder refuses what the walk refuses)
        else:
            assert res[i] == sz[i], (c["name"], res[i], sz[i])       # ... and with the slack it accepts what the walk accepts
            want = D.decode(c["bytes"], int(sz[i]) + batch.LZ4_SIZE_SLACK, d)
            assert want[0] == sz[i] and out[int(ooff[i]):int(ooff[i]) + int(sz[i])].tobytes() == want[1], c["name"]
    # compress on the same stream, then decode what was written: a round trip that never leaves HBM
    raws = [D.words(s, 80 + k) for k, s in enumerate((0, 13, 300, 4096, 16384, 65536, 65537))]
    buf, off, ln = DB.pack(raws, mis=0, dtype=np.int64)
    bound = np.array([len(r) + len(r) // 255 + 16 + 4 for r in raws], np.int64)
    coff = np.concatenate([[0], np.cumsum(bound)[:-1]]).astype(np.int64)
    with torch.cuda.stream(side):
        t_raw = torch.from_numpy(buf).cuda()
        t = [torch.from_numpy(a).cuda() for a in (off, ln, coff, bound)]
        t_comp = torch.zeros(int(bound.sum()) + 64, dtype=torch.uint8, device="cuda")
        cres, dres = (torch.empty(len(raws), dtype=torch.int64, device="cuda") for _ in range(2))
        batch.lz4_compress_blocks_device(t_raw, t[0], t[1], t_comp, t[2], t[3], result=cres, stream=side.cuda_stream, sync=False, dictionary=t_dict)
        clen = cres.clamp(min=0)
        t_back = torch.zeros(int(ln.sum()) + 64, dtype=torch.uint8, device="cuda")
        boff = t[1].cumsum(0) - t[1]
        batch.lz4_decompress_blocks_device(t_comp, t[2], clen, t_back, boff, t[1], store_size=True, result=dres, stream=side.cuda_stream, dictionary=t_dict)
        back, boff = t_back.cpu().numpy(), boff.cpu().numpy()
    side.synchronize()
    cres, dres = cres.cpu().numpy(), dres.cpu().numpy()
    assert cres[-1] == D.INPUT_TOO_LARGE and (cres[:-1] > 4).all(), cres
    for i, r in enumerate(raws[:-1]):
        assert dres[i] == len(r) and back[int(boff[i]):int(boff[i]) + len(r)].tobytes() == r, i
    assert dres[-1] == D.NO_PREFIX                                    # (the refused chunk's stream has length 0)


if __name__ == "__main__":
    dictionary_calls()
    print("dictionary: ok")
