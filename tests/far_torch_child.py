"""Child process of tests/test_far_offsets_gpu.py: batch.lz4_decompress_blocks_device and batch.parquet_decompress_chunks_device on
torch uint8 tensors of the far allocations' size with int64 offset, length, capacity and result tensors, the chunks at places B
(across 2^32) and D (from 2^32 + 2^25 + 5) — what the Python wrappers do to 64-bit rows.  The far runner of tests/device_batch.py does
the rest on an engine object made of torch calls.  torch is imported BEFORE cramjam_amd (tests/device_api_child.py says why)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import device_batch as DB  # noqa: E402
import far_cases as FC  # noqa: E402
from cramjam_amd import batch  # noqa: E402

BITS = 32


class TorchEngine:
    """alloc / free / h2d / d2h / memset / sync of the harness on torch tensors; at(): the tensor view behind a device pointer"""

    def __init__(self):
        self.live = {}

    def alloc(self, nbytes):
        t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
        self.live[t.data_ptr()] = t
        return t.data_ptr()

    def free(self, p):
        del self.live[p]

    def at(self, p, nbytes):
        base = max(b for b in self.live if b <= p)
        assert p - base + nbytes <= self.live[base].numel()
        return self.live[base][p - base:p - base + nbytes]

    def h2d(self, p, data):
        a = np.array(data, copy=True).reshape(-1).view(np.uint8)
        self.at(p, a.nbytes).copy_(torch.from_numpy(a))

    def d2h(self, p, nbytes, dtype="uint8"):
        return self.at(p, nbytes).cpu().numpy().view(dtype).copy()

    def memset(self, p, value, nbytes):
        self.at(p, nbytes).fill_(value)

    def sync(self):
        torch.cuda.synchronize()


def main():
    eng = TorchEngine()
    with DB.far_buffers(eng, BITS) as far:
        half = 1 << (BITS - 1)
        v_in, v_out = eng.at(far.d_in, far.size - half), eng.at(far.d_out, far.size - half)      # the views that begin at the bases
        assert v_in.data_ptr() == far.d_in and v_out.data_ptr() == far.d_out and v_in.numel() > 1 << BITS

        def wrapper(fn, **kw):
            def call(idx, d_in, in_off, in_len, d_out, out_off, out_cap, result):
                rows = [eng.at(p, 8 * len(idx)).view(torch.int64) for p in (in_off, in_len, out_off, out_cap, result)]
                assert int(rows[0].max()) > 1 << BITS and int(rows[2].max()) > 1 << BITS
                assert fn(v_in, rows[0], rows[1], v_out, rows[2], rows[3], result=rows[4], **kw) is rows[4]
            return call
        for name, call in (("lz4-decode", wrapper(batch.lz4_decompress_blocks_device)),
                           ("parquet_snappy-decode", wrapper(batch.parquet_decompress_chunks_device, codec="snappy", verify_crc=True))):
            d = FC.far_list(name)
            DB.run_far(eng, far, name, d["cases"], call, FC.tag_of(name), calls=(("B", "D"),))
    assert not eng.live


if __name__ == "__main__":
    main()
    print("far torch: ok")
