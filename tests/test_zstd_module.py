"""cramjam_amd.zstd / cramjam.zstd: the reference's one-shot calls on the two frame batches with a batch of one.  The
stub and the signatures need no device; the round trips are marked gpu."""
import ast
import inspect
import os

import numpy as np
import pytest

import zstd_enc_cases as E

ROOT = E.ROOT


def test_stub_and_signatures():
    import cramjam
    import cramjam_amd
    assert cramjam.zstd is cramjam_amd.zstd and cramjam.zstd.compress is cramjam_amd.zstd.compress
    from cramjam.zstd import decompress_into  # noqa: F401  (the submodule import resolves through the shim)
    tree = ast.parse(open(os.path.join(ROOT, "cramjam", "zstd.pyi")).read())
    funcs = {n.name: [a.arg for a in n.args.args] for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert set(funcs) == set(cramjam.zstd.__all__) == {"compress", "decompress", "compress_into", "decompress_into"}
    for name, args in funcs.items():
        assert list(inspect.signature(getattr(cramjam.zstd, name)).parameters) == args, name
    assert funcs["compress"] == ["data", "level", "output_len"] and funcs["decompress"] == ["data", "output_len"]
    assert funcs["compress_into"] == ["input", "output", "level"] and funcs["decompress_into"] == ["input", "output"]
    assert not hasattr(cramjam.zstd, "Compressor") and not hasattr(cramjam.zstd, "Decompressor")      # streaming is out of scope
    assert "zstd" in cramjam.__all__ and "zstd" in cramjam_amd.__all__
    for bad in ("3", 3.0, True):
        with pytest.raises(TypeError):
            cramjam.zstd.compress(b"abc", level=bad)
        with pytest.raises(TypeError):
            cramjam.zstd.compress_into(b"abc", bytearray(64), level=bad)


@pytest.mark.gpu
def test_round_trips_over_every_input_type():
    import cramjam
    data = E.cases()["text4k"]
    want = E.model(data)[1]
    for inp in (data, bytearray(data), cramjam.Buffer(data), np.frombuffer(data, np.uint8), np.frombuffer(data, np.uint32), memoryview(data)):
        c = cramjam.zstd.compress(inp)
        assert isinstance(c, cramjam.Buffer) and bytes(c) == want
        d = cramjam.zstd.decompress(c)
        assert isinstance(d, cramjam.Buffer) and bytes(d) == data
    for name in ("len0", "len1", "one65537", "random65792", "text_random_text"):
        data = E.cases()[name]
        c = cramjam.zstd.compress(data)
        assert bytes(c) == E.model(data)[1] and bytes(cramjam.zstd.decompress(bytes(c))) == data, name


@pytest.mark.gpu
def test_into_forms_output_len_and_level(tmp_path):
    import cramjam
    data = E.cases()["text4k"]
    want = E.model(data)[1]
    out = bytearray(b"\xa5" * (len(want) + 32))
    assert cramjam.zstd.compress_into(data, out) == len(want) and bytes(out[:len(want)]) == want and bytes(out[len(want):]) == b"\xa5" * 32
    back = np.full(len(data) + 16, 0xA5, np.uint8)
    assert cramjam.zstd.decompress_into(want, back) == len(data) and back[:len(data)].tobytes() == data and (back[len(data):] == 0xA5).all()
    buf = cramjam.Buffer(bytes(len(data)))
    assert cramjam.zstd.decompress_into(want, buf) == len(data) and bytes(buf) == data
    # output_len is the capacity: honoured, and too small a one is an error of the call's own kind
    assert bytes(cramjam.zstd.compress(data, output_len=len(want))) == want
    with pytest.raises(cramjam.CompressionError, match="CJ_E_OUT_TOO_SMALL"):
        cramjam.zstd.compress(data, output_len=len(want) - 1)
    assert bytes(cramjam.zstd.decompress(want, output_len=len(data))) == data
    assert bytes(cramjam.zstd.decompress(want, output_len=len(data) + 100)) == data
    with pytest.raises(cramjam.DecompressionError, match="CJ_E_OUT_TOO_SMALL"):
        cramjam.zstd.decompress(want, output_len=len(data) - 1)
    with pytest.raises(cramjam.CompressionError):
        cramjam.zstd.compress_into(data, bytearray(10))
    # one level: the bytes do not depend on it
    assert bytes(cramjam.zstd.compress(data, level=3)) == bytes(cramjam.zstd.compress(data, level=None)) == bytes(cramjam.zstd.compress(data, 19)) == want
    # a File: read from its cursor, written through its write()
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as f:
        f.write(data)
    assert bytes(cramjam.zstd.compress(cramjam.File(path))) == want
    fo = cramjam.File(str(tmp_path / "out.zst"))
    assert cramjam.zstd.compress_into(data, fo) == len(want)
    with open(str(tmp_path / "out.zst"), "rb") as f:
        assert f.read() == want


@pytest.mark.gpu
def test_errors_carry_the_code_names():
    import cramjam
    want = E.model(E.cases()["text4k"], 1)[1]
    with pytest.raises(cramjam.DecompressionError, match="CJ_E_ZSTD_SRC_SIZE"):
        cramjam.zstd.decompress(want[:-7])                                  # a truncated frame
    with pytest.raises(cramjam.DecompressionError, match="CJ_E_ZSTD_HEADER"):
        cramjam.zstd.decompress(b"\x00" * 16)
    broken = bytearray(want)
    broken[-1] ^= 1
    with pytest.raises(cramjam.DecompressionError, match="CJ_E_ZSTD_CHECKSUM"):
        cramjam.zstd.decompress(bytes(broken))
    with pytest.raises(cramjam.DecompressionError):
        cramjam.zstd.decompress_into(want[:-7], bytearray(8192))
