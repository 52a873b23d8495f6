# cramjam.zstd — stubs written from cramjam_amd/zstd.py, whose signatures follow the reference's one-shot calls (src/cramjam/zstd.pyi).
# The streaming Compressor / Decompressor of the reference's module are out of scope and not here.
from typing import Optional

from . import Buffer, BytesType

def compress(data: BytesType, level: Optional[int] = None, output_len: Optional[int] = None) -> Buffer:
    """Zstandard compression: one frame with Frame_Content_Size, independent pieces of 64 KiB (any Zstandard decoder reads it).
    There is one compression level: `level` is accepted (an int or None) and does not change the bytes."""
def decompress(data: BytesType, output_len: Optional[int] = None) -> Buffer:
    """Zstandard decompression: what libzstd's ZSTD_decompress reads.  output_len=None: the decoded size is asked for first."""
def compress_into(input: BytesType, output: BytesType, level: Optional[int] = None) -> int:
    """Compress directly into an output buffer; returns the frame's length.  `level` does not change the bytes."""
def decompress_into(input: BytesType, output: BytesType) -> int:
    """Decompress directly into an output buffer; returns the decoded length."""
