"""The public surface of the Blosc chunk support without a GPU: module and enum names, keyword parsing of every stubbed function,
the pure-host helpers (max_compressed_len, cj_blosc_chunk_info), argument checks of the batch entry points and — where there is no
device — CJ_E_NO_DEVICE / RuntimeError from every compute entry (never a CPU result)."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

import blosc_cases as K
import blosc_model as M

ROOT = K.ROOT


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_modules_and_names():
    import cramjam
    import cramjam.experimental
    import cramjam.experimental.blosc2 as b2
    import cramjam_amd
    from cramjam.experimental.blosc2 import compress_chunk
    assert b2 is cramjam_amd.blosc2 and cramjam.experimental.blosc2 is b2 and compress_chunk is cramjam_amd.blosc2.compress_chunk
    for n in ("compress_chunk", "compress_chunk_into", "decompress_chunk", "decompress_chunk_into", "max_compressed_len", "Filter", "CLevel", "Codec"):
        assert hasattr(b2, n), n
    assert not hasattr(cramjam_amd.lz4, "compress_chunk") and not hasattr(cramjam_amd.snappy, "compress_chunk")


def test_enums_have_the_reference_names_and_compare_to_ints():
    from cramjam_amd.blosc2 import CLevel, Codec, Filter
    assert [m.name for m in Filter] == ["NoFilter", "Shuffle", "BitShuffle", "Delta", "TruncPrec", "LastFilter", "LastRegisteredFilter"]
    assert [m.name for m in CLevel] == ["Zero", "One", "Two", "Three", "Four", "Five", "Six", "Seven", "Eight", "Nine"]
    assert [m.name for m in Codec] == ["BloscLz", "LZ4", "LZ4HC", "ZLIB", "ZSTD", "LastCodec", "LastRegisteredCodec"]
    assert Filter.Shuffle == 1 and Filter.BitShuffle == 2 and CLevel.Nine == 9 and Codec.LZ4 == 1 and Codec.BloscLz == 0
    assert Filter.NoFilter != Filter.Shuffle and int(CLevel.Five) == 5


def test_stub_functions_exist_and_accept_their_keywords():
    import cramjam_amd.blosc2 as b2
    tree = ast.parse(open(os.path.join(ROOT, "cramjam", "blosc2.pyi")).read())
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    classes = [n for n in tree.body if isinstance(n, ast.ClassDef)]
    assert {f.name for f in funcs} | {c.name for c in classes} == set(b2.__all__)
    chunk = K.valid()[0]["bytes"]
    for f in funcs:
        fn = getattr(b2, f.name)
        kwargs = {}
        for i, a in enumerate(f.args.args):
            kwargs[a.arg] = (1000 if f.name == "max_compressed_len" else chunk) if i == 0 else (bytearray(1 << 16) if a.arg == "output" else None)
        try:
            fn(**kwargs)
        except TypeError as e:
            pytest.fail("blosc2.%s%r: %s" % (f.name, tuple(kwargs), e))
        except Exception:
            pass                                           # no device: parsing succeeded
    for c in classes:
        members = [t.targets[0].id for t in c.body if isinstance(t, ast.Assign)]
        assert members == [m.name for m in getattr(b2, c.name)], c.name


def test_max_compressed_len():
    import cramjam_amd.blosc2 as b2
    from cramjam_amd import _native as N
    for n in (0, 1, 1000, 1 << 30):
        assert b2.max_compressed_len(n) == n + 32 >= n + 16
        assert N.lib().cj_blosc_chunk_max_compressed_len(n) == n + 32


def _info(b):
    from cramjam_amd import _native as N
    info = N.BloscInfo()
    a = np.frombuffer(b, np.uint8)
    rc = N.lib().cj_blosc_chunk_info(a.ctypes.data if a.size else None, a.size, C.byref(info))
    return rc, info


def test_chunk_info_on_fixtures_and_malformed_headers():
    from cramjam_amd import _native as N
    for v in K.doc()["valid"]:
        rc, info = _info(v["bytes"])
        if not v["supported"]:
            assert rc == N.E_BLOSC_UNSUPPORTED, v["name"]
            continue
        h, _ = M.parse(v["bytes"])
        assert rc == 0 and info.nbytes == v["nbytes"] == h["nbytes"] and info.cbytes == len(v["bytes"]), v["name"]
        assert (info.typesize, info.flags, info.blocksize, info.nblocks) == (h["typesize"], h["flags"], h["blocksize"], h["nblocks"]), v["name"]
    seen = set()
    for m in K.malformed():
        rc, _ = _info(m["bytes"])
        try:
            M.parse(m["bytes"])
            want = None
        except M.Refused as r:
            want = M.CODE[r.cls]
        # the header checks are a prefix of the walk: an error they report is the model's; one that only the walk finds shows as 0 here
        assert rc in (0, N.E_BLOSC_HEADER, N.E_BLOSC_UNSUPPORTED) and (rc == 0 or rc == want), (m["name"], rc, want)
        seen.add(rc)
    assert seen == {0, N.E_BLOSC_HEADER, N.E_BLOSC_UNSUPPORTED}
    assert "blosc" in N.strerror(N.E_BLOSC_HEADER) and "unsupported" in N.strerror(N.E_BLOSC_UNSUPPORTED)
    assert N.strerror(N.E_BLOSC_HEADER) != N.strerror(N.E_BLOSC_UNSUPPORTED)
    assert N.lib().cj_blosc_chunk_info(None, 0, None) == -101


def test_batch_argument_checks_need_no_device():
    from cramjam_amd import _native as N
    from cramjam_amd import batch, blosc2
    L = N.lib()
    # n == 0 succeeds everywhere, bad arguments are refused before any device is looked for
    assert L.cj_blosc_chunk_sizes_host(None, 0, 0, None, None, None) == 0
    assert L.cj_blosc_chunk_sizes_host(None, 1, 0, None, None, None) == -101          # flags are reserved
    assert L.cj_blosc_chunk_sizes_host(None, 0, 1, None, None, None) == -101          # null pointers with n > 0
    assert L.cj_blosc_chunk_sizes_device(None, 0, 0, None, None, None, None, None) == 0
    assert L.cj_blosc_chunk_sizes_device(None, 0, 3, None, None, None, None, None) == -101
    assert L.cj_blosc_batch_host(None, 0, 0, 0, None, None, None, None, None, None) == 0
    assert L.cj_blosc_batch_host(None, 7, 0, 0, None, None, None, None, None, None) == -101         # unknown op
    assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, None) == -101         # compress without params
    assert L.cj_blosc_batch_host(None, 0, 0, 3, None, None, None, None, None, None) == -101         # null pointers with n > 0
    assert L.cj_blosc_batch_device(None, 0, None, None, None, None, None, None, None, 0, None, 0, None) == 0
    assert L.cj_blosc_batch_device(None, 7, None, None, None, None, None, None, None, 0, None, 0, None) == -101
    assert L.cj_blosc_batch_device(None, 0, None, None, None, None, None, None, None, 3, None, 0, None) == -101
    for bad, want in ((N.BloscParams(0, 1, 5, 1, 0), -101), (N.BloscParams(256, 1, 5, 1, 0), -101), (N.BloscParams(4, 1, 10, 1, 0), -101),
                      (N.BloscParams(4, 3, 5, 1, 0), N.E_BLOSC_UNSUPPORTED), (N.BloscParams(4, 4, 5, 1, 0), N.E_BLOSC_UNSUPPORTED),
                      (N.BloscParams(4, 1, 5, 0, 0), N.E_BLOSC_UNSUPPORTED), (N.BloscParams(4, 1, 5, 3, 0), N.E_BLOSC_UNSUPPORTED),
                      (N.BloscParams(4, 1, 5, 4, 0), N.E_BLOSC_UNSUPPORTED)):
        assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(bad)) == want
        assert L.cj_blosc_batch_device(None, 1, None, None, None, None, None, None, None, 0, C.byref(bad), 0, None) == want
    ok = N.BloscParams(4, 1, 5, 2, 0)                                                               # LZ4HC: the same streams
    assert L.cj_blosc_batch_host(None, 1, 0, 0, None, None, None, None, None, C.byref(ok)) == 0
    with pytest.raises(ValueError):
        blosc2.compress_chunk(b"abcd", typesize=0)
    with pytest.raises(ValueError):
        blosc2.compress_chunk(b"abcd", typesize=4, clevel=12)
    with pytest.raises(TypeError):
        batch.blosc_chunk_sizes_device([1, 2, 3], [0], [3])                                         # not a device buffer


def test_typesize_defaults_to_the_itemsize_of_the_buffer():
    from cramjam_amd import blosc2
    assert blosc2._view(b"abcdefgh")[1] == 1
    assert blosc2._view(np.zeros(8, np.float32))[1] == 4 and blosc2._view(np.zeros((2, 4), np.float64))[1] == 8
    assert blosc2._view(np.zeros(8, np.float32))[0].nbytes == 32
    assert blosc2._params(None, None, None, None).typesize == 1 and blosc2._params(None, None, None, None).codec == blosc2.Codec.LZ4


def test_every_compute_entry_fails_without_a_device():
    if not _no_gpu():
        return
    from cramjam_amd import _native as N
    from cramjam_amd import batch, blosc2
    L = N.lib()
    chunk = K.valid()[0]["bytes"]
    out = C.create_string_buffer(1 << 16)
    p = N.BloscParams(4, 1, 5, 1, 0)
    assert L.cj_blosc_chunk_decompress(chunk, len(chunk), C.cast(out, C.c_void_p), 1 << 16) == N.E_NO_DEVICE
    assert L.cj_blosc_chunk_compress(b"abcd" * 64, 256, C.cast(out, C.c_void_p), 1 << 16, C.byref(p)) == N.E_NO_DEVICE
    ptrs, lens, res = (C.c_void_p * 1)(C.cast(C.c_char_p(chunk), C.c_void_p)), (C.c_size_t * 1)(len(chunk)), (C.c_int64 * 1)()
    assert L.cj_blosc_chunk_sizes_host(None, 0, 1, ptrs, lens, res) == N.E_NO_DEVICE
    for call in (lambda: blosc2.compress_chunk(b"abcd" * 64), lambda: blosc2.compress_chunk_into(b"abcd" * 64, bytearray(512)),
                 lambda: blosc2.decompress_chunk(chunk), lambda: blosc2.decompress_chunk_into(chunk, bytearray(1 << 16)),
                 lambda: batch.blosc_decompress_chunks([chunk]), lambda: batch.blosc_compress_chunks([b"abcd" * 64], 4),
                 lambda: batch.blosc_chunk_sizes([chunk])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "no usable HIP device" in str(e.value)
