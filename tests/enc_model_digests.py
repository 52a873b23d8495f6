"""The scalar encoder models' outputs as digests (tests/golden/enc_model_digests.json): the seeded inputs and the walk over every model
entry that tests/golden/make_enc_model_digests.py records and tests/test_enc_model_digests.py repeats.  The inputs are small but reach
every branch of the matcher's round (tests/hostsim/enc2_round.h): the first partial round and the span's doubling, a last block of 128
that is cut short, the lap of the 16-bit table, followers of a run of equal distances, and the distance limit.  Data and helpers only;
nothing here needs a GPU."""
import ctypes as C
import hashlib

import deflate_cases as D
import deflate_enc_cases as DE
import oracle
import zstd_enc_cases as ZE
from test_enc2_linked_model import linked_lib
from test_enc2_model import model_lib

SYNTH_LENS = (0, 7, 8, 12, 13, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 140000)
ROUNDS = (256, 512, 1024)
HISTORIES = (0, 1, 4096, 65536)
FAR = ((0, 65528), (100, 32768), (200, 32769))      # (a 16-byte marker's position, the distance to its repeat)


def far_input():
    """70 000 bytes whose matches, apart from the runs of zeros between them, lie 32 768, 32 769 and 65 528 back: deflate_enc_cases'
    distance_case for three markers at once — zeros in between, so that the table keeps each marker until its repeat comes.  The
    repeat 65 528 back begins at the last position of the first piece at which a match may start."""
    out = bytearray(70000)
    for k, (at, d) in enumerate(FAR):
        m = bytes(1 + b % 255 for b in D.random_bytes(16, 4000 + k))
        out[at:at + 16] = m
        out[at + d:at + d + 16] = m
    return bytes(out)


def inputs():
    """[(name, data)]"""
    ins = [("synth%d" % n, oracle.synth_v1(n, k)) for k, n in enumerate(SYNTH_LENS)]
    ins.append(("one_byte", b"\x5a" * 70000))
    ins.append(("period3", (b"abc" * 23334)[:70000]))
    ins.append(("far", far_input()))
    return ins


def _entry(r, buf):
    return [int(r), hashlib.sha256(bytes(buf[:max(int(r), 0)])).hexdigest()]


def digests():
    """entry -> {input name: [returned length, SHA-256 of the output]} of the models as they are built now"""
    E2, EL, LD, LZ = model_lib(), linked_lib(), DE.lib(), ZE.lib()
    out = {}
    for name, data in inputs():
        n = len(data)
        buf = C.create_string_buffer(n + n // 6 + 64)
        for R in ROUNDS:
            out.setdefault("enc2_model_lz4/R%d" % R, {})[name] = _entry(E2.enc2_model_lz4(data, n, buf, R), buf)
            out.setdefault("enc2_model_snappy/R%d" % R, {})[name] = _entry(E2.enc2_model_snappy(data, n, buf, R), buf)
        for h in HISTORIES:
            if n >= h:                                   # (the block behind the history: at most 64 KiB)
                m = min(n, h + 65536)
                out.setdefault("enc2_model_lz4_linked/h%d" % h, {})[name] = _entry(EL.enc2_model_lz4_linked(data, h, m, buf, 512), buf)
        for wrap in DE.WRAPS:
            r, s, _, _ = DE.model(data, wrap)
            out.setdefault("dfe_model_compress/%s" % DE.WRAP_NAME[wrap], {})[name] = _entry(r, s)
        for flags in ZE.FLAGS:
            r, s, _ = ZE.model(data, flags)
            out.setdefault("zse_model_compress/flags%d" % flags, {})[name] = _entry(r, s)
    return out
