"""Decoded-size queries (cj_batch_sizes_*, cj_frame_batch_sizes_*, cramjam_amd.batch.*_sizes*) without a GPU: the scalar size walk of the
kernels (cramjam_amd/csrc/lz4_size_walk.hpp) compiled for the host as a stand-alone program under AddressSanitizer + UBSan and held
to the oracle's decoder with unlimited room; CJ_LZ4_SIZE_SLACK held to the oracle; the argument rules of the exports and of the
Python functions.  (The compute side is tests/test_batch_sizes_gpu.py.)"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import batch_sizes_cases as K
from conftest import ROOT
from cramjam_amd import _native as N
from cramjam_amd import batch
from hostsim_build import build_sim

SIM_DIR = os.path.join(ROOT, "tests", "hostsim")
SIM = os.path.join(SIM_DIR, "sim_lz4_size_walk")


@pytest.fixture(scope="module")
def walked():
    """[(tag, block, from_encoder, the host walk's answer)] for every case"""
    build_sim("sim_lz4_size_walk.cpp", SIM, main=True, sanitize=True, extra=["-static-libasan"])
    cases = K.lz4_cases()
    feed = b"".join(struct.pack("<I", len(b)) + b for _, b, _ in cases)
    r = subprocess.run([SIM], input=feed, capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    return [(t, b, e, g) for (t, b, e), g in zip(cases, got)]


def test_the_scalar_size_walk_is_the_oracles_decoder_with_unlimited_room(walked):
    bad = [(t, len(b), g, K.expected_size(b)) for t, b, _, g in walked if g != K.expected_size(b)]
    assert not bad, bad[:10]
    # the cases cover what they are meant to: accepted and rejected blocks, the 64-bit path, blocks on both sides of 64 KiB
    assert sum(g >= 0 for _, _, _, g in walked) > 300 and sum(g == K.E_CORRUPT for _, _, _, g in walked) > 200
    assert [g for t, _, _, g in walked if t == ("huge-match",)] == [K.E_PREFIX_TOO_BIG]
    assert any(len(b) > (1 << 20) for _, b, _, _ in walked) and any(len(b) == 0 for _, b, _, _ in walked)


def test_twelve_bytes_of_slack_decode_every_accepted_block(walked):
    """CJ_LZ4_SIZE_SLACK against the ORACLE's decoder (not ours): cap = S + 12 gives S for every accepted block, cap = S for every
    block that came out of an encoder"""
    assert K.SLACK == batch.LZ4_SIZE_SLACK == 12
    assert "#define CJ_LZ4_SIZE_SLACK 12" in open(os.path.join(ROOT, "include", "cramjam_hip.h")).read()
    n_ok = 0
    for t, b, enc, g in walked:
        if g < 0:
            continue
        n_ok += 1
        assert K.oracle_decode(b, g + K.SLACK) == g, (t, g)
        if enc:
            assert K.oracle_decode(b, g) == g, (t, g)
    assert n_ok > 300


def test_argument_rules_of_the_exports():
    L = N.lib()
    dev = (L.cj_batch_sizes_device, L.cj_frame_batch_sizes_device)
    host = (L.cj_batch_sizes_host, L.cj_frame_batch_sizes_host)
    one = (C.c_uint64 * 2)()
    p = C.cast(one, C.c_void_p)
    for k, fn in enumerate(dev):
        assert fn(None, 0, 0, 0, None, None, None, None, None) == 0                           # n == 0 succeeds
        assert fn(None, 1, 0, 0, None, None, None, None, None) == 0
        assert fn(None, 2, 0, 0, None, None, None, None, None) == -101                        # unknown codec / format
        assert fn(None, -1, 0, 1, p, p, p, p, None) == -101
        assert fn(None, 0, 2, 0, None, None, None, None, None) == -101                        # a flag bit that is not the prefix
        assert fn(None, 0, 0x100, 1, p, p, p, p, None) == -101
        assert fn(None, 0, 1, 0, None, None, None, None, None) == (0 if k == 0 else -101)     # the prefix flag means something for blocks only
        for hole in range(4):                                                                  # a null pointer with n > 0
            args = [p, p, p, p]
            args[hole] = None
            assert fn(None, 0, 0, 1, *args, None) == -101
    for k, fn in enumerate(host):
        assert fn(None, 0, 0, 0, None, None, None) == 0
        assert fn(None, 2, 0, 0, None, None, None) == -101
        assert fn(None, 0, 4, 0, None, None, None) == -101
        assert fn(None, 0, 1, 0, None, None, None) == (0 if k == 0 else -101)
        assert fn(None, 0, 0, 1, None, p, p) == -101 and fn(None, 0, 0, 1, p, None, p) == -101 and fn(None, 0, 0, 1, p, p, None) == -101
    import torch
    if not torch.cuda.is_available():                       # no device: no CPU answer either
        ptrs = (C.c_void_p * 1)(C.cast(C.c_char_p(b"\x00"), C.c_void_p))
        lens = (C.c_size_t * 1)(1)
        res = (C.c_int64 * 1)(77)
        for fn in host:
            assert fn(None, 0, 0, 1, ptrs, lens, res) == N.E_NO_DEVICE and res[0] == 77
        for fn in dev:
            assert fn(None, 0, 0, 1, p, p, p, p, None) == N.E_NO_DEVICE


class FakeDev:
    def __init__(self, shape, typestr="|u1", ptr=0x7000_0000_0000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}


SIZES_DEVICE = ("lz4_block_sizes_device", "snappy_raw_sizes_device", "lz4_frame_bounds_device", "snappy_framed_sizes_device")


@pytest.mark.parametrize("name", SIZES_DEVICE)
def test_device_functions_refuse_what_the_decode_functions_refuse(name, monkeypatch):
    fn = getattr(batch, name)
    buf = FakeDev((1 << 16,))
    with pytest.raises(ValueError):
        fn(buf, [0], [10], stream=0)                                        # the NULL stream cannot be named
    for host_obj in (b"abc", bytearray(8), [1, 2, 3]):
        with pytest.raises(TypeError):
            fn(host_obj, [0], [3])                                          # host bytes are not a device buffer
    with pytest.raises(ValueError):
        fn(np.zeros(16, np.uint8), [0], [3])                                # numpy's DLPack capsule says "CPU"

    class NoEngine:                                                         # (metadata is looked at once an engine exists: one that never touches a device)
        h = None
        def alloc(self, n): raise AssertionError("nothing may be uploaded for device-resident metadata")
        def free(self, p): pass
    monkeypatch.setattr(batch, "_engine", lambda device: NoEngine())
    with pytest.raises(TypeError):
        fn(buf, FakeDev((4,), "<u4"), FakeDev((4,), "<u4"), result=FakeDev((4,), "<i8"))        # 32-bit metadata
    with pytest.raises(ValueError):
        fn(buf, FakeDev((4,), "<u8"), FakeDev((5,), "<u8"), result=FakeDev((4,), "<i8"))        # ragged metadata
    with pytest.raises(ValueError):
        fn(buf, FakeDev((4,), "<u8"), FakeDev((4,), "<u8"), result=FakeDev((4,), "<i4"))        # a 32-bit result


def test_the_existing_decode_signature_still_takes_its_lengths_by_position():
    import inspect
    sig = inspect.signature(batch.lz4_decompress_blocks)
    assert list(sig.parameters)[:3] == ["blocks", "output_lens", "store_size"] and sig.parameters["output_lens"].default is None
    for name in ("lz4_block_sizes", "snappy_raw_sizes", "lz4_frame_bounds", "snappy_framed_sizes"):
        assert callable(getattr(batch, name))
