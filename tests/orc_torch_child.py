"""Child process of tests/test_orc_gpu.py: orc_compress_streams_device on torch tensors on a side stream, then orc_stream_sizes_device
and orc_decompress_streams_device over what it wrote, with the encoder's device results as the decoder's in_len; then the golden streams
of one codec through the device entries with host metadata.  torch is imported BEFORE cramjam_amd, as a user of both has to
(tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import orc_model as M  # noqa: E402
import device_batch as DB  # noqa: E402
import deflate_cases as D  # noqa: E402
from cramjam_amd import batch  # noqa: E402

BS = 65536


def round_trip(codec, give_result):
    text = D.words(150000, 93)
    rnd = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    chunks = [text[:n] for n in (0, 1, 4000, BS, BS + 1, 150000)] + [rnd]
    n = len(chunks)
    buf, off, ln = DB.pack(chunks, mis=0, dtype=np.int64)
    cap = np.array([batch.orc_compress_bound(int(x), BS) for x in ln], np.int64)
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
        got = batch.orc_compress_streams_device(t_in, t_off, t_len, t_out, t_ooff, t_cap, codec, BS, result=res, stream=side.cuda_stream, sync=False)
        clen = res if give_result else torch.from_numpy(np.asarray(got, np.int64)).cuda()
        assert not give_result or got is res
        batch.orc_stream_sizes_device(t_out, t_ooff, clen, codec, BS, result=res3, stream=side.cuda_stream, sync=False)
        batch.orc_decompress_streams_device(t_out, t_ooff, clen, t_back, t_off, t_len, codec, BS, result=res2, stream=side.cuda_stream, sync=False)
    side.synchronize()
    clen, res2, res3, out, back = clen.cpu().numpy(), res2.cpu().numpy(), res3.cpu().numpy(), t_out.cpu().numpy(), t_back.cpu().numpy()
    for i, c in enumerate(chunks):
        s = out[int(ooff[i]):int(ooff[i]) + int(clen[i])].tobytes()
        assert clen[i] >= 0, (codec, i, clen[i])
        M.check_encoded(s, c, BS, codec, random_input=c is rnd)
        assert res2[i] == res3[i] == len(c) and back[int(off[i]):int(off[i]) + len(c)].tobytes() == c, (codec, i, res2[i], res3[i])


def golden_streams(codec):
    gs = M.golden_of(codec, BS)
    streams = [g["stream"] for g in gs]
    buf, off, ln = DB.pack(streams, mis=0, dtype=np.int64)
    sizes = np.array([g["decoded_len"] for g in gs], np.int64)
    ooff = np.concatenate([[0], np.cumsum(sizes + 16)[:-1]]).astype(np.int64)
    t_in = torch.from_numpy(buf).cuda()
    t_out = torch.zeros(int((sizes + 16).sum()) + 64, dtype=torch.uint8, device="cuda")
    assert list(batch.orc_stream_sizes_device(t_in, off, ln, codec, BS)) == list(sizes)
    res = batch.orc_decompress_streams_device(t_in, off, ln, t_out, ooff, sizes, codec, BS)
    out = t_out.cpu().numpy()
    for i, g in enumerate(gs):
        assert res[i] == sizes[i] and M.digest(out[int(ooff[i]):int(ooff[i]) + int(sizes[i])]) == g["sha256"], (codec, g["name"], res[i])


if __name__ == "__main__":
    for k, codec in enumerate(M.KINDS):
        round_trip(codec, k % 2 == 0)
        golden_streams(codec)
    print("orc torch: ok")
