"""Decoded-size queries on the GPU (cj_batch_sizes_*, cj_frame_batch_sizes_*, cramjam_amd.batch.*_sizes*): raw LZ4 blocks walked to
their end and held to the oracle's decoder with unlimited room — golden vectors, malformed streams, fuzz, the corpus, chunks of
1 B .. 5 MiB and empty ones, at odd byte offsets, as batches of 1 .. 24 576; the contract with the decoder (capacity S + 12 for every
accepted block, S for every encoder's output) with both calls queued on one stream; the header and frame queries against the
single-buffer exports and the oracle; the host variants and lz4_decompress_blocks without output_lens; a frame query next to a
queued frame batch.  The checks run in ONE child process (tests/batch_sizes_child.py) that imports torch first.

Measured with this test's inputs (MI355X): see DESIGN.md 5.9 for the rates."""
import os

import pytest

import device_batch as DB

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_decoded_size_queries_from_torch_tensors():
    pytest.importorskip("torch")
    DB.run_child(os.path.join(HERE, "batch_sizes_child.py"), "batch sizes: ok", 1500)
