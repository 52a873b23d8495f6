"""BGZF (SAM specification 4.1) for the tests: a writer on zlib's raw DEFLATE to the layout cramjam_hip.h states, the walk over the
members' heads and the stream-order verdict as a Python model, and the seeded case list of tests/test_bgzf_model.py and
tests/test_bgzf_gpu.py.  No htslib-written file was available; every stream here comes from the writer below."""
import struct
import zlib

import deflate_cases as D

BAD_ARG, INPUT_TOO_LARGE, PREFIX_TOO_BIG, OUT_TOO_SMALL = -101, -1, -5, -6
CORRUPT, HEADER, CHECKSUM, EOF, TRAILING = D.CORRUPT, D.HEADER, D.CHECKSUM, D.EOF, D.TRAILING
PIECE = 0xff00
MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- the writer ---------------------------------------------------------------------------------------------------------------------
def member(piece, level=6, pre=b"", post=b"", fname=None):
    """one member: FLG = FEXTRA (| FNAME), MTIME 0, XFL 0, OS 255, the subfields pre | BC 2 BSIZE | post, raw DEFLATE, CRC32, ISIZE"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(piece) + c.flush()
    xlen = len(pre) + 6 + len(post)
    name = b"" if fname is None else fname + b"\0"
    total = 12 + xlen + len(name) + len(body) + 8
    assert total <= 65536
    head = struct.pack("<BBBBIBBH", 31, 139, 8, 4 | (8 if fname is not None else 0), 0, 0, 255, xlen)
    return head + pre + b"BC" + struct.pack("<HH", 2, total - 1) + post + name + body + struct.pack("<II", zlib.crc32(piece), len(piece))


def subfield(si, payload):
    return si + struct.pack("<H", len(payload)) + payload


def stream(pieces, level=6, marker=True, **kw):
    return b"".join(member(p, level, **kw) for p in pieces) + (MARKER if marker else b"")


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def walk(s):
    """(code, [(offset, length, isize)]): cj::bgzf_walk — the members visited before the first error, and that error or 0"""
    s, pos, out = bytes(s), 0, []
    n = len(s)
    while pos < n:
        left = n - pos
        if left < 12:
            return EOF, out
        xlen = s[pos + 10] | s[pos + 11] << 8
        if left < 12 + xlen:
            return EOF, out
        if s[pos] != 31 or s[pos + 1] != 139 or s[pos + 2] != 8 or not s[pos + 3] & 4:
            return HEADER, out
        x, q, bsize = s[pos + 12:pos + 12 + xlen], 0, None
        while q < xlen:
            if xlen - q < 4:
                return HEADER, out
            slen = x[q + 2] | x[q + 3] << 8
            if slen > xlen - q - 4:
                return HEADER, out
            if bsize is None and x[q:q + 2] == b"BC" and slen == 2:
                bsize = x[q + 4] | x[q + 5] << 8
            q += 4 + slen
        if bsize is None:
            return HEADER, out
        ln = bsize + 1
        if ln < 12 + xlen + 2 + 8:
            return HEADER, out
        if ln > left:
            return EOF, out
        out.append((pos, ln, struct.unpack_from("<I", s, pos + ln - 4)[0]))
        pos += ln
    return 0, out


def sizes(s):
    """what the size query says: the ISIZE sum or the walk's error"""
    code, mem = walk(s)
    return code if code else sum(m[2] for m in mem)


def decode(s, cap=None):
    """(code or total, bytes): the walk's error first; CJ_E_OUT_TOO_SMALL when the ISIZE sum exceeds cap (None: the sum itself); then the
    first member in stream order that zlib refuses at a capacity of its own ISIZE — a member that holds more than that is
    CJ_E_DEFLATE_CHECKSUM, zlib's "incorrect length check".  An error's bytes are empty."""
    s = bytes(s)
    code, mem = walk(s)
    if code:
        return code, b""
    total = sum(m[2] for m in mem)
    if cap is not None and total > cap:
        return OUT_TOO_SMALL, b""
    outs = []
    for off, ln, isize in mem:
        if isize > 0x7E000000:
            return PREFIX_TOO_BIG, b""
        r, o = D.verdict(D.GZIP, s[off:off + ln], isize)
        if r < 0:
            return (CHECKSUM if r == OUT_TOO_SMALL else r), b""
        outs.append(o)
    return total, b"".join(outs)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
_pool = None


def _text(n, seed):
    """n bytes of word-like text: a slice, by the seed, of one pool (deflate_cases.words)"""
    global _pool
    if _pool is None:
        _pool = D.words(200000, 5)
    at = seed * 7919 % (len(_pool) - n)
    return _pool[at:at + n]


def _patch(s, at, b):
    return s[:at] + bytes(b) + s[at + len(b):]


def _bsize_at(s, off):
    """offset of the BSIZE field of the member at off (a member of the writer without foreign subfields in front)"""
    assert s[off + 12:off + 14] == b"BC"
    return off + 16


_cases = None


def cases():
    """name -> (family, stream).  Families of valid streams begin with "ok"."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    # valid: levels 0, 1, 9 (stored, fixed and dynamic blocks) over streams of 0, 1, 2, 64, 65 and 300 members
    for k, nm in enumerate((0, 1, 2, 64, 65, 300)):
        for level in (0, 1, 9):
            pieces = [_text(40 + (37 * i + 11 * nm) % 500, 1000 * nm + i) for i in range(nm)]
            c["ok_members%d_level%d" % (nm, level)] = ("ok", stream(pieces, level, marker=(k + level) % 2 == 0))
    big = [_text(30000, 7), _text(PIECE, 8), D.random_bytes(5000, 9)]
    for level in (0, 1, 9):
        c["ok_big_level%d" % level] = ("ok", stream(big, level))
    a, b = _text(700, 21), _text(1300, 22)
    c["ok_empty_first"] = ("ok", stream([b"", a, b], marker=False))
    c["ok_empty_middle"] = ("ok", stream([a, b"", b"", b]))
    c["ok_empty_last"] = ("ok", stream([a, b, b""], marker=False))
    c["ok_marker_only"] = ("ok", MARKER)
    c["ok_marker_in_front"] = ("ok", MARKER + stream([a]))
    c["ok_no_marker"] = ("ok", stream([a, b], marker=False))
    c["ok_foreign_before"] = ("ok", stream([a, b], pre=subfield(b"XY", b"\x01\x02\x03")))
    c["ok_foreign_after"] = ("ok", stream([a, b], post=subfield(b"ZZ", b"")))
    c["ok_foreign_both"] = ("ok", stream([a, b], pre=subfield(b"BD", b"\xff" * 5), post=subfield(b"CB", b"\x00\x00")))
    c["ok_bc_slen4_then_bc"] = ("ok", stream([a], pre=subfield(b"BC", b"\x09\x09\x09\x09")))      # (the first BC of two bytes counts)
    c["ok_fname"] = ("ok", stream([a, b], fname=b"reads.bam"))
    c["ok_incompressible_full_piece"] = ("ok", stream([D.random_bytes(PIECE, 31)]))
    c["ok_incompressible_full_piece_stored"] = ("ok", stream([D.random_bytes(PIECE, 31)], 0))
    c["ok_two_full_pieces_and_a_byte"] = ("ok", stream([D.random_bytes(PIECE, 32), _text(PIECE, 33), b"x"], 1))

    # malformed.  Truncation at every byte of a two-member stream (a cut at a member boundary is a valid stream)
    two = stream([b"hello, blocked gzip", _text(90, 41)], marker=False)
    ends = {0} | {m[0] + m[1] for m in walk(two)[1]}
    for cut in range(len(two)):
        c["cut_%03d" % cut] = ("ok_cut" if cut in ends else "cut", two[:cut])
    m0, m1 = walk(two)[1]
    for name, at, delta in (("first", m0[0], 1), ("first", m0[0], -1), ("last", m1[0], 1), ("last", m1[0], -1)):
        p = _bsize_at(two, at)
        v = struct.unpack_from("<H", two, p)[0] + delta
        c["bsize_%s_%+d" % (name, delta)] = ("bc", _patch(two, p, struct.pack("<H", v)))
    c["bsize_below_minimum"] = ("bc", _patch(two, _bsize_at(two, m1[0]), struct.pack("<H", 12 + 6 + 2 + 8 - 2)))
    c["bsize_zero"] = ("bc", _patch(two, _bsize_at(two, 0), b"\0\0"))
    c["bsize_past_end"] = ("bc", _patch(two, _bsize_at(two, m1[0]), struct.pack("<H", m1[1] - 1 + 100)))
    one = member(a)
    body = one[18:]
    head = lambda extra: one[:10] + struct.pack("<H", len(extra)) + extra
    fix = lambda h: _patch(h + body, 0, h)          # (BSIZE is not mended: these die before it is looked at, or on it)
    c["bc_slen4"] = ("bc", fix(head(subfield(b"BC", struct.pack("<HH", len(one) + 1, 0)))))
    c["bc_missing"] = ("bc", fix(head(subfield(b"XY", struct.pack("<H", len(one) - 1)))))
    c["bc_wrong_si2"] = ("bc", fix(head(subfield(b"BD", struct.pack("<H", len(one) - 1)))))
    c["slen_past_xlen"] = ("bc", _patch(one, 14, struct.pack("<H", 3)))
    c["slen_past_xlen_foreign"] = ("bc", stream([a], pre=b"XY\x09\x00"))
    c["subfield_head_cut"] = ("bc", stream([a], post=b"XY\x00"))
    c["fextra_clear"] = ("magic", _patch(stream([a]), 3, b"\0"))
    c["cm_7"] = ("magic", _patch(stream([a]), 2, b"\x07"))
    c["bad_magic_member2"] = ("magic", _patch(two, m1[0] + 1, b"\x8c"))
    three = stream([_text(3000, 51), _text(2000, 52), _text(1000, 53)], 9)
    mem3 = walk(three)[1]
    for k in (0, 1, 2):
        off, ln, _ = mem3[k]
        c["crc_bit_member%d" % k] = ("crc", _patch(three, off + ln - 8, bytes([three[off + ln - 8] ^ 0x10])))
        for delta in (1, -1):
            v = struct.pack("<I", mem3[k][2] + delta)
            c["isize_member%d_%+d" % (k, delta)] = ("isize", _patch(three, off + ln - 4, v))
    off, ln, _ = mem3[1]
    for j, bit in enumerate((0, 3, 17, 40, 171, 1000, 4001, 6007)):           # (not the last byte's unused bits: those are no damage)
        at = off + 18 + bit // 8
        c["data_bit_%d" % j] = ("data", _patch(three, at, bytes([three[at] ^ (1 << bit % 8)])))
    stored = stream([_text(500, 61), _text(600, 62)], 0)
    c["data_stored_len"] = ("data", _patch(stored, 18 + 1, bytes([stored[19] ^ 1])))
    c["zero_padding_3"] = ("zero_padding", stream([a, b]) + b"\0\0\0")
    c["zero_padding_3_no_marker"] = ("zero_padding", stream([a, b], marker=False) + b"\0\0\0")
    c["garbage_byte"] = ("garbage", stream([a, b]) + b"\x5a")
    c["garbage_byte_no_marker"] = ("garbage", stream([a], marker=False) + b"\x5a")
    _cases = c
    return c


_want = {}


def want(name):
    """decode() of a case at the capacity of its own ISIZE sum, computed once"""
    if name not in _want:
        _want[name] = decode(cases()[name][1])
    return _want[name]


def compress_bound(n):
    """cj_bgzf_compress_bound from the DEFLATE bound: the members' gzip bounds with the 18-byte header for the 10-byte one, and the marker"""
    if n > 0x7E000000:
        return 0
    gz = lambda p: p + 10 * (p // 65536) + 5 + 18
    full, rest = divmod(n, PIECE)
    return full * (gz(PIECE) + 8) + (gz(rest) + 8 if rest else 0) + 28
