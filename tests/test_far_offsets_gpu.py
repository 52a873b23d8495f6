"""Device batches placed beyond 4 GiB (tests/device_batch.py: the far placement): every device entry, both directions,
with both 64-bit offset rows around 2^31, across 2^32, exactly at 2^32 and at 2^32 + 2^25 + 5, on two allocations of 6.06 GiB made
once for this module (12.2 GiB at the peak).  The case lists are subsets of the suite's own (tests/far_cases.py), so every expected
value is the reference's; what is new is where the chunks lie.  A kernel that cut an offset to 32 bits anywhere between the row and
the pointer addition reads a decoy or writes a shadow window inside the allocations: an assertion that names the chunk, not a fault."""
import os

import pytest

import device_batch as DB
import far_cases as FC
from capacity_cases import PATHS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS = ("lz4-decode", "snappy-decode")


@pytest.fixture(scope="module")
def eng():
    from cramjam_amd.batch import _engine
    return _engine(0)


@pytest.fixture(scope="module")
def far(eng):
    with DB.far_buffers(eng, 32) as f:
        yield f


def run(eng, far, name, *call_args):
    d = FC.far_list(name)
    DB.run_far(eng, far, name, d["cases"], d["call"](eng, *call_args), FC.tag_of(name), dictionary=d["dictionary"])


@pytest.mark.parametrize("flags,win", PATHS)
@pytest.mark.parametrize("name", BLOCKS)
def test_block_decoders(eng, far, name, flags, win):
    """the lane, wave, fused and parse-kernel mappings and the three windows"""
    run(eng, far, name, flags)


@pytest.mark.parametrize("name", sorted(set(FC.LISTS) - set(BLOCKS)))
def test_far(eng, far, name):
    run(eng, far, name)


def test_the_python_wrappers_on_torch_tensors():
    """lz4_decompress_blocks_device and parquet_decompress_chunks_device with int64 offset tensors at places B and D, in a child that
    imports torch BEFORE cramjam_amd"""
    pytest.importorskip("torch")
    DB.run_child(os.path.join(HERE, "far_torch_child.py"), "far torch: ok", 600)
