"""CPU model of BloscLZ streams inside Blosc1 chunks (c-blosc 1.21 blosclz_decompress): test infrastructure, not product code.
The stream decoder in plain Python, a chunk decoder on top of blosc_model.parse (the container is the one blosc_model walks; only
the compressor format differs), `wrap` for chunks around hand-written streams, the hand-written streams themselves, and the loader
of tests/golden/golden_blosclz.json + .bin."""
import hashlib
import json
import os
import struct

import numpy as np

import blosc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = 2                                     # CJ_BLOSC_FLAG_READ_BLOSCLZ


def decode_stream(src, cap):
    """the `cap` decoded bytes of one stream, or Refused(corrupt).  Every index is checked here; nothing relies on Python's slicing."""
    src = bytes(src)
    n = len(src)

    def bad(why):
        return M.Refused(M.CORRUPT, "blosclz: " + why)
    if n == 0:
        raise bad("empty")
    out = bytearray()
    ip = 1
    ctrl = src[0] & 31
    while True:
        if ctrl < 32:
            run = ctrl + 1
            if len(out) + run > cap or ip + run > n:
                raise bad("literal run")
            out += src[ip:ip + run]
            ip += run
            if ip >= n:
                break
            ctrl = src[ip]; ip += 1
            continue
        ln, ofs = (ctrl >> 5) - 1, (ctrl & 31) << 8
        if ln == 6:
            while True:
                if ip + 1 >= n:
                    raise bad("length bytes")
                code = src[ip]; ip += 1
                ln += code
                if code != 255:
                    break
        elif ip + 1 >= n:
            raise bad("match at the end")
        code = src[ip]; ip += 1
        ln += 3
        dist = ofs + code
        if code == 255 and ofs == 31 << 8:
            if ip + 1 >= n:
                raise bad("far distance")
            dist = (src[ip] << 8) + src[ip + 1] + 8191
            ip += 2
        dist += 1
        if len(out) + ln > cap:
            raise bad("match past the capacity")
        if dist > len(out):
            raise bad("distance before the start")
        last = ip >= n
        if not last:
            ctrl = src[ip]; ip += 1
        if dist >= ln:
            out += out[len(out) - dist:len(out) - dist + ln]
        else:                                                  # overlapping: the last `dist` bytes repeat
            pat = bytes(out[len(out) - dist:])
            out += (pat * (ln // dist + 1))[:ln]
        if last:
            break
    if len(out) != cap:
        raise bad("decoded %d of %d" % (len(out), cap))
    return bytes(out)


def is_blosclz(chunk):
    """a chunk whose streams are BloscLZ: format 0, versionlz 1, not memcpyed (what the default reading refuses as unsupported)"""
    return len(chunk) >= 16 and chunk[0] == 2 and chunk[1] == 1 and chunk[2] >> 5 == 0 and not chunk[2] & 2


def parse(chunk):
    """blosc_model.parse with the BloscLZ format admitted: the format bits are rewritten for the parse only, the chunk is not altered"""
    chunk = bytes(chunk)
    if not is_blosclz(chunk):
        return M.parse(chunk)
    seen = bytearray(chunk)
    seen[2] |= 1 << 5
    h, streams = M.parse(bytes(seen))
    h["flags"] = chunk[2]
    return h, streams


def decode(chunk, cap=None):
    """the plain bytes of a chunk read with the flag on (LZ4 chunks go to blosc_model.decode), or Refused"""
    chunk = bytes(chunk)
    if not is_blosclz(chunk):
        return M.decode(chunk, cap)
    h, streams = parse(chunk)
    n = h["nbytes"]
    if cap is not None and n > cap:
        raise M.Refused(M.TOO_SMALL)
    if n == 0:
        return b""
    image = bytearray(n)
    for src, ln, dst, dlen, _b, stored in streams:
        assert 16 <= src and src + ln <= len(chunk) and dst + dlen <= n
        image[dst:dst + dlen] = chunk[src:src + ln] if stored else decode_stream(chunk[src:src + ln], dlen)
    bs = h["blocksize"]
    out = bytearray()
    for at in range(0, n, bs):
        blk = image[at:at + bs]
        out += M.apply_filter(blk, h["typesize"], M.block_mode(h["flags"], h["typesize"], len(blk)), False)
    return bytes(out)


def verdict(chunk, cap=None):
    try:
        return "ok", decode(chunk, cap)
    except M.Refused as r:
        return r.cls, None


# ---- chunks around hand-written streams -------------------------------------------------------------------------------------------
def wrap(streams, typesize, each, filter_flags=0):
    """a valid Blosc1 chunk (format BloscLZ) around `streams`, every one of which decodes to `each` bytes.  typesize 1: unsplit blocks
    of one stream; typesize > 1: split blocks of typesize streams (len(streams) a multiple of typesize).  filter_flags: 0, 1 or 4."""
    per = typesize if typesize > 1 else 1
    assert streams and len(streams) % per == 0 and all(len(s) != each for s in streams), "a stream of exactly its decoded length reads as stored"
    nblocks = len(streams) // per
    blocksize = per * each
    body, starts = bytearray(), []
    at = 16 + 4 * nblocks
    for b in range(nblocks):
        starts.append(at + len(body))
        for s in streams[b * per:(b + 1) * per]:
            body += struct.pack("<i", len(s)) + bytes(s)
    flags = filter_flags | (0 if typesize > 1 else 16)
    total = at + len(body)
    return struct.pack("<BBBBIII", 2, 1, flags, typesize, nblocks * blocksize, blocksize, total) + struct.pack("<%dI" % nblocks, *starts) + bytes(body)


def lit(data):
    out = bytearray()
    for k in range(0, len(data), 32):
        run = data[k:k + 32]
        out += bytes([len(run) - 1]) + run
    return bytes(out)


def match(ln, dist):
    """the bytes of a match of ln >= 3 bytes at distance dist >= 1 (without a control byte behind it)"""
    assert ln >= 3 and 1 <= dist <= 73727
    d, far = dist - 1, b""
    if d >= 8191:
        far = struct.pack(">H", d - 8191)
        d = 8191
    k = ln - 3
    ext = b""
    if k >= 6:
        rest = k - 6
        ext = b"\xff" * (rest // 255) + bytes([rest % 255])
        k = 6
    return bytes([((k + 1) << 5) | (d >> 8)]) + ext + bytes([d & 255]) + far


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def hand_streams():
    """[(name, stream, cap)]: the edges of the stream grammar; the verdict of each is the model's (decode_stream)"""
    R = _noise(80000, 77)
    tail = lit(b"xyz")
    c = []
    c.append(("dist_8191_plain", lit(R[:8200]) + match(5, 8191) + tail, 8208))                      # ofs = 31 << 8, code = 254
    c.append(("code_255_not_far", lit(R[:8000]) + match(5, 30 * 256 + 256) + tail, 8008))           # code = 255, ofs = 30 << 8
    c.append(("far_0000", lit(R[:8192]) + match(4, 8192) + tail, 8199))
    c.append(("far_0000_one_short", lit(R[:8191]) + match(4, 8192) + tail, 8198))                   # dist == op + 1: bad
    c.append(("far_ffff_at_op", lit(R[:73727]) + match(7, 73727) + tail, 73737))
    c.append(("far_ffff_one_short", lit(R[:73726]) + match(7, 73727) + tail, 73736))                # bad
    c.append(("len_ext_ff_ff_00", lit(R[:100]) + bytes([0xE0, 255, 255, 0, 49]) + tail, 100 + 519 + 3))
    c.append(("match_ends_at_cap", lit(R[:40]) + match(20, 7), 60))
    c.append(("match_one_over_cap", lit(R[:40]) + match(20, 7), 59))                                # bad
    c.append(("far_match_ends_at_cap", lit(R[:9000]) + match(5, 8500), 9005))
    c.append(("run_match_ends_at_cap", lit(R[:3]) + match(5000, 1), 5003))                          # distance 1: a byte run to the last byte
    c.append(("literals_end_at_n", lit(R[:40]), 40))
    c.append(("literals_one_short", lit(R[:40])[:-1], 40))                                          # bad
    c.append(("lone_match_control", lit(R[:40]) + b"\x40", 44))                                     # bad
    c.append(("lone_long_match_control", lit(R[:40]) + b"\xe0", 49))                                # bad
    c.append(("match_without_its_code", lit(R[:40]) + b"\x40\x05", 43))                             # two bytes are needed behind the control: bad
    c.append(("dist_equals_op", lit(R[:10]) + match(5, 10) + tail, 18))
    c.append(("dist_op_plus_1", lit(R[:10]) + match(5, 11) + tail, 18))                             # bad
    c.append(("first_byte_e0_k", bytes([0xE0 | 9]) + R[:10] + match(5, 3) + tail, 18))              # the first control & 31: 10 literals
    c.append(("short_of_cap", lit(R[:40]), 41))                                                     # bad: ends before its capacity
    c.append(("overlap_d65", lit(R[:65]) + match(1000, 65) + tail, 1068))
    c.append(("overlap_d3", lit(R[:7]) + match(300, 3) + tail, 310))
    # a stream above 256 KiB (libblosc cuts its blocks at 256 KiB, so none of the minted streams is): a distance-1 run of 265 000
    # bytes, literals, then a far match whose output lies beyond byte 262 144 and whose source straddles the run's end
    c.append(("above_256k_run_then_far_match", lit(R[:3]) + match(265000, 1) + lit(R[3:60003]) + match(50, 60040) + tail, 3 + 265000 + 60000 + 50 + 3))
    return c


def hand_chunks():
    """[dict(name, bytes, verdict, out)]: every hand-written stream as a chunk of its own (typesize 1, one unsplit block), and three
    chunks of four streams behind the byte shuffle whose streams end in matches: they lie back to back in the decoder's scratch"""
    out = []
    for name, s, cap in hand_streams():
        out.append(dict(name=name, bytes=wrap([s], 1, cap)))
    R = _noise(4096, 78)
    four = [lit(R[k * 50:k * 50 + 24 + k]) + match(64 - 24 - k, 5 + k) for k in range(4)]
    out.append(dict(name="split4_end_in_matches", bytes=wrap(four, 4, 64, 1)))
    out.append(dict(name="split4_two_blocks", bytes=wrap(four + four[::-1], 4, 64, 1)))
    over = list(four)
    over[1] = lit(R[50:50 + 25]) + match(64 - 25 + 1, 6)                                            # one byte into its neighbour's place: bad
    out.append(dict(name="split4_second_one_over", bytes=wrap(over, 4, 64, 1)))
    for e in out:
        e["verdict"], e["out"] = verdict(e["bytes"])
    return out


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
_doc = None


def doc():
    global _doc
    if _doc is None:
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosclz.json")) as f:
            _doc = json.load(f)
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosclz.bin"), "rb") as f:
            blob = f.read()
        for i, v in enumerate(_doc["valid"]):
            v["name"] = M.name_of(v["recipe"], i)
            v["bytes"] = blob[v["at"]:v["at"] + v["len"]]
        for m in _doc["malformed"]:
            m["bytes"] = M.mutate(_doc["valid"][m["base"]]["bytes"], m["mutation"])
    return _doc


def valid():
    return doc()["valid"]


def malformed():
    return doc()["malformed"]


def raw_of(v):
    r = v["recipe"]
    return M.make_input(r["kind"], r["size"], r["seed"])


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()
