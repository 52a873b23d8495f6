"""Batches of framed streams (cj_frame_batch_device / cj_frame_batch_host): the exports and the Python calls exist, are bound, and
refuse cleanly — without a device, the Python calls raise as the block calls do.  No GPU needed."""
import ctypes as C

import pytest

from cramjam_amd import _native as N
from cramjam_amd import batch


def test_frame_batch_exports_are_bound():
    assert {"cj_frame_batch_device", "cj_frame_batch_host"} <= set(N.SYMBOLS)
    assert (N.FORMAT_LZ4_FRAME, N.FORMAT_SNAPPY_FRAMED) == (0, 1)
    assert "cj_debug_xxh32_device" in N.BENCH_SYMBOLS


def test_null_engine_and_bad_arguments_are_refused():
    L = N.lib()
    one = (C.c_uint64 * 1)(0)
    res = (C.c_int64 * 1)(0)
    ptrs = (C.c_void_p * 1)(None)
    lens = (C.c_size_t * 1)(0)
    for fmt in (0, 1):
        for op in (0, 1):
            assert L.cj_frame_batch_device(None, fmt, op, 0, 1, None, one, one, None, one, one, res, None) < 0
            assert L.cj_frame_batch_host(None, fmt, op, 0, 1, ptrs, lens, ptrs, lens, res) < 0
    assert L.cj_frame_batch_host(None, 0, 0, 0, 0, None, None, None, None, None) == N.lib().cj_frame_batch_host(None, 7, 0, 0, 0, None, None, None, None, None)
    assert L.cj_frame_batch_host(None, 0, 0, 0, 0, None, None, None, None, None) == -101 == L.cj_frame_batch_device(None, 0, 0, 0, 0, None, None, None, None, None, None, None, None)
    if L.cj_device_count() > 0:                 # behind the engine check: an empty batch, a flag, a format, an op, a host batch without a row
        e = batch._engine(0).h
        dev = lambda fmt, op, flags: L.cj_frame_batch_device(e, fmt, op, flags, 0, None, None, None, None, None, None, None, None)
        host = lambda fmt, op, flags, n=0, rows=(None,) * 5: L.cj_frame_batch_host(e, fmt, op, flags, n, *rows)
        for call in (dev, host):
            assert [call(fmt, op, 0) for fmt in (0, 1) for op in (0, 1)] == [0] * 4
            assert call(0, 0, 1) == -101 and call(7, 0, 0) == -101 and call(0, 2, 0) == -101
        full = (ptrs, lens, ptrs, lens, res)
        for hole in range(5):
            assert host(0, 0, 0, 1, full[:hole] + (None,) + full[hole + 1:]) == -101


def test_host_frame_calls_raise_without_a_device():
    if N.lib().cj_device_count() > 0:
        return                                  # (a device is present: tests/test_frame_batch_gpu.py covers the calls)
    for call, arg in ((batch.lz4_decompress_frames, [b"\x04\x22\x4d\x18"]), (batch.lz4_compress_frames, [b"abc"]),
                      (batch.snappy_decompress_framed_many, [b"\xff\x06\x00\x00sNaPpY"]), (batch.snappy_compress_framed_many, [b"abc"])):
        with pytest.raises(RuntimeError):
            call(arg)
