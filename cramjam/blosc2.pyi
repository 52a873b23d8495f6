# Stub of cramjam.experimental.blosc2 (= cramjam_amd.blosc2): the chunk API of the reference's blosc2 module, written from
# cramjam_amd/blosc2.py's own signatures.
from enum import IntEnum
from typing import Optional

from . import Buffer, BytesType

class Filter(IntEnum):
    NoFilter = 0
    Shuffle = 1
    BitShuffle = 2
    Delta = 3
    TruncPrec = 4
    LastFilter = 5
    LastRegisteredFilter = 6

class CLevel(IntEnum):
    Zero = 0
    One = 1
    Two = 2
    Three = 3
    Four = 4
    Five = 5
    Six = 6
    Seven = 7
    Eight = 8
    Nine = 9

class Codec(IntEnum):
    BloscLz = 0
    LZ4 = 1
    LZ4HC = 2
    ZLIB = 3
    ZSTD = 4
    LastCodec = 5
    LastRegisteredCodec = 6

def compress_chunk(data: BytesType, typesize: Optional[int] = None, clevel: Optional[CLevel] = None, filter: Optional[Filter] = None, codec: Optional[Codec] = None) -> Buffer: ...
def compress_chunk_into(input: BytesType, output: BytesType, typesize: Optional[int] = None, clevel: Optional[CLevel] = None, filter: Optional[Filter] = None, codec: Optional[Codec] = None) -> int: ...
def decompress_chunk(data: BytesType, output_len: Optional[int] = None, blosclz: bool = False, zlib: bool = False, zstd: bool = False) -> Buffer: ...
def decompress_chunk_into(input: BytesType, output: BytesType, blosclz: bool = False, zlib: bool = False, zstd: bool = False) -> int: ...
def max_compressed_len(len_bytes: int) -> int: ...
