"""What the tests of an engine's shared scratch areas submit, and what the references say comes out: tests/test_scratch_streams_model.py
(no GPU) checks this module, tests/scratch_streams_child.py runs its pairings on two caller streams, tests/test_scratch_turn_gpu.py
takes its newer cases from it.  One Call is one batch for one device entry of cramjam_amd.batch; one Pairing is a call X for stream
`a` and a call Y for stream `b` that share a scratch of cj_engine (csrc/cj_engine.hpp), with the debug budgets that make both run
many slices over the same three slots.

Inputs come from the case modules the codecs already have, expectations from their references: the oracle (LZ4 / Snappy blocks and
frames, golden_vectors.json's malformed blocks), zlib / gzip and deflate_enc_cases.model / bgzf_model (DEFLATE, BGZF),
zstd_enc_cases.model and the recorded verdicts of zstd_cases (Zstandard), the recorded fixtures of blosc_cases / blosc_zcodec_model
(Blosc), test_enc2_linked_model.model_linked (the dictionary encoder).  Malformed inputs sit between the good ones; none makes a CALL
fail.

SLICES.  A scratch with a budget holds `slots` slots; a call of n streams runs ceil(n / slots) kernel launches over them, each slice
on slots 0 .. slots - 1 again.  The slot sizes are those include/cramjam_hip_debug.h states.  `scratch` (the workgroup decoders'
verdict rows and chunk counter) and `fb` (the container batches' tables, rows and data scratch) have no budget: every call lays its
tables out from the buffers' first byte, so any two calls collide on all of it — Pairing.slices is None there, and the argument is
that layout."""
import base64
import gzip
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

G = 64                      # guard bytes around every output slot
FILL = 0xA5
MIN_SLICES = 8

# bytes of one slot, as include/cramjam_hip_debug.h states them
ZSTD_SLOT = 128 * 1024 + 32
ZSTD_ENC_SLOT = 320 * 1024 + 256            # 320.25 KiB
DEFLATE_SLOT = 256 * 1024 + 256             # 256.25 KiB
BGZF_SLOT = 65312
DICT_LEN = 4096
DICT_SLOT = (DICT_LEN + 65536 + 255) & ~255     # `dictionary tail | chunk`: the tail that counts, a chunk of at most 64 KiB, 256-byte granules
SLOTS = 3                                   # the budget of a pairing's scratch, in slots ...
BGZF_SLOTS = 2                              # ... and of the BGZF members' slots inside `fb`

OUT_TOO_SMALL, INPUT_TOO_LARGE, LZ4_CORRUPT = -6, -1, -7


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- what a chunk must give -----------------------------------------------------------------------------------------------------------
class Want:
    """result and bytes of one chunk by its reference: `data` (exact bytes, result = their length), `digest` (sha256 of `size` bytes),
    `code` (an exact negative result), `negative` (some negative result: the reference refuses, its code is its own) or `verify`
    (bytes -> bool for an encoder whose bytes no reference pins: the reference's decoder reads them back)"""

    def __init__(self, data=None, size=None, digest=None, code=None, negative=False, verify=None):
        self.data, self.size, self.digest, self.code, self.negative, self.verify = data, size, digest, code, negative, verify
        if data is not None:
            self.size = len(data)

    @property
    def good(self):
        return self.code is None and not self.negative

    def problem(self, result, slot):
        """None, or what is wrong with `result` and the chunk's slot (its `capacity` bytes)"""
        result = int(result)
        if self.negative:
            return None if result < 0 else "result %d, the reference refuses" % result
        if self.code is not None:
            return None if result == self.code else "result %d, want %d" % (result, self.code)
        if self.verify is not None:
            return None if result > 0 and self.verify(bytes(slot[:result])) else "result %d: the reference does not read it back" % result
        if result != self.size:
            return "result %d, want %d" % (result, self.size)
        got = bytes(slot[:result])
        if self.data is not None and got != self.data:
            return "bytes differ from the reference's at %d" % next(i for i in range(result) if got[i] != self.data[i])
        if self.digest is not None and sha(got) != self.digest:
            return "sha256 differs from the recorded one"
        return None


class Call:
    """one batch: entry = the name of the device entry in cramjam_amd.batch, kw = its keyword arguments besides the buffers;
    flags / codec (LZ4 and Snappy blocks only): the call goes through cj_batch_device with these; host = the name of the host entry
    (the mode with a host batch beside a device batch); dictionary: bytes"""

    def __init__(self, label, entry, chunks, caps, want, kw=None, flags=None, codec=None, host=None, dictionary=None):
        assert len(chunks) == len(caps) == len(want) and chunks
        self.label, self.entry, self.chunks, self.caps, self.want = label, entry, [bytes(c) for c in chunks], [int(c) for c in caps], want
        self.kw, self.flags, self.codec, self.host, self.dictionary = kw or {}, flags, codec, host, dictionary

    @property
    def n(self):
        return len(self.chunks)

    def times(self, k):
        """the same batch k times over (more work per call, the same slots)"""
        return Call(self.label, self.entry, self.chunks * k, self.caps * k, self.want * k, self.kw, self.flags, self.codec, self.host, self.dictionary)

    def layout(self):
        """(input blob size, in_off, in_len, out_off, total output bytes): chunks 16 bytes apart, slot i G bytes behind slot i - 1's end"""
        off, run = [], 0
        for c in self.chunks:
            off.append(run); run += (len(c) + 15) // 16 * 16 + 16
        ooff, orun = [], G
        for c in self.caps:
            ooff.append(orun); orun += c + G
        return run + 64, off, [len(c) for c in self.chunks], ooff, orun + 64

    def problems(self, res, out, ooff):
        """every chunk against its Want, and every byte outside [slot, slot + result) of a good chunk — or outside the slot of a
        refused one — still FILL; out: a numpy uint8 array of the whole output buffer.  A list of (chunk, text)."""
        import numpy as np
        bad = []
        keep = np.ones(out.size, bool)
        for i, (w, o, cap) in enumerate(zip(self.want, ooff, self.caps)):
            p = w.problem(res[i], out[o:o + cap])
            if p:
                bad.append((i, p))
            used = max(int(res[i]), 0) if w.good else cap       # (a refused chunk may have written inside its slot before it was found out)
            keep[o:o + min(used, cap)] = False
        if not (out[keep] == FILL).all():
            at = int(np.flatnonzero(keep & (out != FILL))[0])
            bad.append((-1, "a write outside a chunk's result at byte %d of the output" % at))
        return bad


class Pairing:
    def __init__(self, name, scratch, x, y, budgets=(), slices=None, host_mode=False):
        """budgets: [(name of the cj_debug_* export, bytes)]; slices: (of X, of Y) at those budgets, None for a scratch without one"""
        self.name, self.scratch, self.x, self.y, self.budgets, self.slices, self.host_mode = name, scratch, x, y, list(budgets), slices, host_mode


def _ceil(a, b):
    return -(-a // b)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _once(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    return wrapped


def _golden():
    if "golden" not in _cache:
        with open(os.path.join(HERE, "golden", "golden_vectors.json")) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def _mix(good, bad, every):
    """the items of `bad` between those of `good`, one behind every `every` good ones"""
    out, bad = [], list(bad)
    for i, g in enumerate(good):
        out.append(g)
        if i % every == every - 1 and bad:
            out.append(bad.pop(0))
    return out + bad


@_once
def lz4_blocks(n, size, seed, flags=0):
    """n LZ4 blocks of word-like text by the oracle's encoder, malformed blocks of golden_vectors.json between them (refused: -7)"""
    import lz4_dict_model as D
    import oracle
    good = []
    for k in range(n):
        raw = D.words(size + 7 * (k % 5), seed + k)
        good.append((oracle.lz4_compress_raw(raw)[1], len(raw), Want(data=raw)))
    bad = []
    for m in _golden()["malformed_lz4"][::25]:
        data = base64.b64decode(m["data"])
        r, o = oracle.lz4_decompress_raw(data, m["cap"])
        bad.append((data, m["cap"], Want(code=LZ4_CORRUPT) if r < 0 else Want(data=o)))
    rows = _mix(good, bad, max(1, n // (len(bad) + 1)))
    from cramjam_amd import _native as N
    return Call("LZ4 blocks, decompress" + (", parse kernel" if flags else ""), "lz4_decompress_blocks_device", [r[0] for r in rows], [r[1] for r in rows],
                [r[2] for r in rows], flags=flags, codec=N.CODEC_LZ4_BLOCK, host="lz4_decompress_blocks")


@_once
def snappy_blocks(n, size, seed, flags=0):
    """n Snappy raw blocks by the oracle's encoder, malformed blocks of golden_vectors.json between them (the oracle's own code)"""
    import lz4_dict_model as D
    import oracle
    good = []
    for k in range(n):
        raw = D.words(size + 11 * (k % 7), seed + k)
        good.append((oracle.snappy_compress(raw)[1], len(raw), Want(data=raw)))
    bad = []
    for m in _golden()["malformed_snappy"][::13]:
        data = base64.b64decode(m["data"])
        cap = max(oracle.snappy_decompress_len(data), 0)
        if cap > 70000:
            continue
        r, o = oracle.snappy_decompress(data, cap)
        bad.append((data, cap, Want(code=r) if r < 0 else Want(data=o)))
    rows = _mix(good, bad, max(1, n // (len(bad) + 1)))
    from cramjam_amd import _native as N
    return Call("Snappy raw blocks, decompress" + (", parse kernel" if flags else ""), "snappy_decompress_raw_many_device", [r[0] for r in rows],
                [r[1] for r in rows], [r[2] for r in rows], flags=flags, codec=N.CODEC_SNAPPY_RAW)


@_once
def lz4_frames(n, seed):
    """n LZ4 frames by the oracle's writer: one to four blocks of 64 KiB, every block-size code, with and without block checksums;
    between them frames cut short and frames with a damaged content checksum (the oracle refuses both)"""
    import lz4_dict_model as D
    import oracle
    rows = []
    for k in range(n):
        raw = D.words((3000 + 7 * k, 70000, 140000 + k, 200000)[k % 4], seed + k)
        f = oracle.lz4_frame_compress(raw, 4 + k % 4, (oracle.LZ4F_CONTENT_SIZE, oracle.LZ4F_CONTENT_SIZE | oracle.LZ4F_BLOCK_CHECKSUM)[k % 2])[1]
        assert oracle.lz4_frame_decompress(f, len(raw)) == (len(raw), raw)
        rows.append((f, len(raw), Want(data=raw)))
        if k % 8 == 3:
            rows.append((f[:len(f) - 5], len(raw), Want(negative=True)))
        if k % 8 == 6:
            rows.append((f[:-1] + bytes([f[-1] ^ 0x40]), len(raw), Want(negative=True)))
    for f, cap, w in rows:
        assert not w.negative or oracle.lz4_frame_decompress(f, cap)[0] < 0
    return Call("LZ4 frames, decompress", "lz4_decompress_frames_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


@_once
def snappy_framed_compress(n, seed):
    """n buffers into Snappy framed streams; what comes out is read back by the oracle's reader.  Two capacities of 10 bytes: refused"""
    import lz4_dict_model as D
    import oracle
    from cramjam_amd import _native as N
    L = N.lib()
    rows = []
    for k in range(n):
        raw = D.words((900 + k, 65536, 70001, 150000 + k)[k % 4], seed + k)
        verify = lambda s, raw=raw: oracle.snappy_frame_decompress(s, len(raw)) == (len(raw), raw)
        rows.append((raw, L.cj_snappy_frame_max_compress_len(len(raw)), Want(verify=verify)))
        if k % 6 == 2:
            rows.append((raw, 10, Want(negative=True)))
    return Call("Snappy framed streams, compress", "snappy_compress_framed_many_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


@_once
def blosc_lz4_shuffle():
    """the recorded Blosc chunks with LZ4 streams behind the byte shuffle, their recorded sha256; malformed chunks mutated from them,
    with their recorded verdict's code"""
    import blosc_cases as K
    import blosc_model as M
    every = K.doc()["valid"]                                   # (a malformed chunk names its base by its index here)
    pick = [i for i, v in enumerate(every) if v["supported"] and v["recipe"]["filter"] == 1 and v["nbytes"] <= 300001]
    good = [(every[i]["bytes"], every[i]["nbytes"], Want(size=every[i]["nbytes"], digest=every[i]["sha256"])) for i in pick]
    bad = [(m["bytes"], every[m["base"]]["nbytes"], Want(code=M.CODE[m["verdict"]]))
           for m in K.malformed() if m["base"] in pick and m["verdict"] != "ok"][::9]
    assert len(good) >= 40 and len(bad) >= 6
    rows = _mix(good, bad, max(1, len(good) // (len(bad) + 1)))
    return Call("Blosc chunks (LZ4 streams, shuffle), decompress", "blosc_decompress_chunks_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


@_once
def bgzf_decode():
    """bgzf_model's cases (every fifth of the truncations; not the streams of 300 members: one lane walks a stream's members before the
    call's one wait, which is what submitting this call costs), each with the model's verdict and bytes at the capacity of its ISIZE sum"""
    import bgzf_model as B
    names = [k for k in B.cases() if not k.startswith(("cut_", "ok_members300"))] + [k for k in B.cases() if k.startswith("cut_")][::5]
    rows = []
    for k in names:
        s = B.cases()[k][1]
        r, o = B.want(k)
        rows.append((s, max(B.sizes(s), 0), Want(data=o) if r >= 0 else Want(code=r)))
    return Call("BGZF streams, decompress", "bgzf_decompress_many_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


@_once
def blosc_zstd():
    """the recorded Blosc chunks whose streams are Zstandard frames, and the recorded malformed ones with their verdict's code"""
    import blosc_model as M
    import blosc_zcodec_model as Z
    good = [(v["bytes"], v["nbytes"], Want(size=v["nbytes"], digest=v["sha256"])) for v in Z.valid() if Z.fmt_of(v["bytes"]) == Z.FORMAT_ZSTD]
    bad = [(m["bytes"], m["cap"], Want(code=M.CODE[m["verdict"]])) for m in Z.malformed() if m["name"].startswith("zstd") and m["verdict"] != "ok"][::16]
    rows = _mix(good, bad, max(1, len(good) // (len(bad) + 1)))
    return Call("Blosc chunks (Zstd streams), decompress", "blosc_decompress_chunks_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                kw={"zstd": True})


def blosc_zstd_rows(call):
    """the streams of a Blosc call that go through the Zstandard launcher: the chunks' streams that are not stored, of the chunks the
    walk accepts (a lower bound: the launcher is entered once for the streams of transposed blocks, once for the others)"""
    import blosc_zcodec_model as Z
    return sum(len(Z.streams_of(c)) for c, w in zip(call.chunks, call.want) if w.good)


@_once
def zstd_decode(step):
    """the recorded cases of zstd_cases with at most 64 KiB on either side — every step-th of those libzstd accepts, and between them
    every twelfth of those it refuses: its verdict at its capacity, its sha256"""
    import zstd_cases as ZC
    small = [c for c in ZC.load_cases() if c.cap <= 65536 and 0 < len(c.stream) <= 65536]
    good, bad = [c for c in small if c.accepted][::step], [c for c in small if not c.accepted][::12]
    cs = _mix(good, bad, max(1, len(good) // (len(bad) + 1)))
    want = [Want(size=c.verdicts[0], digest=c.sha) if c.verdicts[0] >= 0 else Want(code=c.verdicts[0]) for c in cs]
    return Call("Zstandard chunks, decompress", "zstd_decompress_many_device", [c.stream for c in cs], [c.cap for c in cs], want, host="zstd_decompress_many")


def _member_payloads_are_the_models(stream, buf):
    """a BGZF stream of `buf`: gzip reads it, its members are the pieces of 65 280 bytes and the marker, and the DEFLATE data of every
    member is deflate_enc_cases.model's for that piece"""
    import bgzf_model as B
    import deflate_enc_cases as E
    if gzip.decompress(stream) != buf or B.decode(stream) != (len(buf), buf):
        return False
    code, mem = B.walk(stream)
    if code != 0 or len(mem) != _ceil(len(buf), B.PIECE) + 1 or stream[mem[-1][0]:] != B.MARKER:
        return False
    for k, (off, ln, isize) in enumerate(mem[:-1]):
        piece = buf[k * B.PIECE:(k + 1) * B.PIECE]
        if isize != len(piece) or stream[off + 18:off + ln - 8] != E.model(piece, E.RAW)[1]:
            return False
    return True


@_once
def bgzf_compress():
    """8 buffers of 3 to 5 members (text, and one incompressible piece among them) into BGZF streams, and one capacity of 100 bytes"""
    import bgzf_model as B
    import deflate_cases as D
    from cramjam_amd import _native as N
    text, rnd = D.words(5 * B.PIECE + 100, 78), D.random_bytes(B.PIECE, 7)
    sizes = (3 * B.PIECE, 2 * B.PIECE + 1, 4 * B.PIECE - 100, 5 * B.PIECE, 2 * B.PIECE + 5000, 3 * B.PIECE + 1, 4 * B.PIECE, 3 * B.PIECE - 1)
    rows = []
    for k, n in enumerate(sizes):
        buf = text[k * 11:k * 11 + n]
        if k == 2:
            buf = buf[:B.PIECE] + rnd + buf[2 * B.PIECE:]
        assert len(buf) == n and 3 <= _ceil(n, B.PIECE) <= 5
        rows.append((buf, N.lib().cj_bgzf_compress_bound(n), Want(verify=lambda s, buf=buf: _member_payloads_are_the_models(s, buf))))
        if k == 4:
            rows.append((buf, 100, Want(code=OUT_TOO_SMALL)))
    return Call("buffers into BGZF streams", "bgzf_compress_many_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


def bgzf_members(call):
    import bgzf_model as B
    return sum(_ceil(len(c), B.PIECE) for c in call.chunks)


@_once
def deflate_zlib_compress():
    """deflate_enc_cases' cases below 70 000 bytes into zlib streams: the model's bytes; every ninth at a capacity one byte short"""
    import deflate_enc_cases as E
    rows = []
    for k, (name, data) in enumerate(sorted(E.cases().items())):
        if len(data) >= 70000:
            continue
        r, s = E.model(data, E.ZLIB)[:2]
        assert r == len(s) > 0
        if k % 9 == 4:
            assert E.model(data, E.ZLIB, r - 1)[0] == OUT_TOO_SMALL
            rows.append((data, r - 1, Want(code=OUT_TOO_SMALL)))
        else:
            rows.append((data, E.bound(len(data), E.ZLIB), Want(data=s)))
    return Call("buffers into zlib streams", "deflate_compress_many_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], kw={"wrapper": "zlib"})


@_once
def zstd_compress(half, checksum):
    """one half (by their order) of zstd_enc_cases' cases below 70 000 bytes into frames: the model's bytes; every ninth one byte short"""
    import zstd_enc_cases as E
    rows = []
    for k, (name, data) in enumerate(list(E.cases().items())[half::2]):
        if len(data) >= 70000:
            continue
        r, s = E.model(data, int(checksum))[:2]
        assert r == len(s) > 0
        if k % 9 == 4:
            assert E.model(data, int(checksum), r - 1)[0] == OUT_TOO_SMALL
            rows.append((data, r - 1, Want(code=OUT_TOO_SMALL)))
        else:
            rows.append((data, E.bound(len(data), int(checksum)), Want(data=s)))
    return Call("buffers into Zstandard frames, %s checksum" % ("with" if checksum else "no"), "zstd_compress_many_device", [r[0] for r in rows],
                [r[1] for r in rows], [r[2] for r in rows], kw={"checksum": bool(checksum)})


@_once
def dict_compress(n, size, seed):
    """n chunks against a 4 096-byte dictionary: the linked encoder's model; one chunk of 65 537 bytes, which the entry refuses (-1)"""
    import lz4_dict_model as D
    from cramjam_amd import _native as N
    from test_enc2_linked_model import linked_lib, model_linked
    d = D.dictionary(DICT_LEN)
    M = linked_lib()
    L = N.lib()
    rows = []
    for k in range(n):
        raw = D.words(size + 13 * (k % 4), seed + k)
        s = model_linked(M, d, raw)
        assert D.decode(s, len(raw), d) == (len(raw), raw)
        rows.append((raw, L.cj_lz4_block_compress_bound(len(raw), 0), Want(data=s)))
        if k == n // 2:
            big = D.words(65537, seed + 999)
            rows.append((big, L.cj_lz4_block_compress_bound(len(big), 0), Want(code=INPUT_TOO_LARGE)))
    return Call("chunks against a dictionary, compress", "lz4_compress_blocks_device", [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
                kw={"store_size": False}, dictionary=d)


# ---- the pairings ---------------------------------------------------------------------------------------------------------------------
def pairings():
    """name -> Pairing, in the order of the issue's table.  Built once."""
    if "pairings" in _cache:
        return _cache["pairings"]
    from cramjam_amd import _native as N
    ps = []
    ps.append(Pairing("P1", "scratch", lz4_blocks(12288, 4096, 9000), snappy_blocks(768, 1500, 9500), host_mode=True))
    ps.append(Pairing("P1k", "scratch", lz4_blocks(12288, 4096, 9000, N.FLAG_FORCE_PARSE_KERNEL), snappy_blocks(768, 1500, 9500, N.FLAG_FORCE_PARSE_KERNEL)))
    ps.append(Pairing("P2", "fb", lz4_frames(48, 12000), snappy_framed_compress(16, 12500)))
    ps.append(Pairing("P3", "fb", blosc_lz4_shuffle().times(2), bgzf_decode()))
    ps.append(Pairing("P4", "fb -> scratch | scratch", lz4_frames(48, 12000), lz4_blocks(1024, 2048, 13000)))
    x, y = blosc_zstd(), zstd_decode(2)
    ps.append(Pairing("P5", "fb -> zstd_slots | zstd_slots", x, y, [("cj_debug_zstd_slot_budget", SLOTS * ZSTD_SLOT)],
                      (_ceil(blosc_zstd_rows(x), SLOTS), _ceil(y.n, SLOTS)), host_mode=True))
    x, y = bgzf_compress(), deflate_zlib_compress()
    # X: every BGZF turn of two members enters the DEFLATE encoder once — one slice of its three slots
    ps.append(Pairing("P6", "fb -> deflate_slots | deflate_slots", x, y,
                      [("cj_debug_bgzf_slot_budget", BGZF_SLOTS * BGZF_SLOT), ("cj_debug_deflate_slot_budget", SLOTS * DEFLATE_SLOT)],
                      (_ceil(bgzf_members(x), BGZF_SLOTS), _ceil(y.n, SLOTS))))
    x, y = zstd_compress(0, False), zstd_compress(1, True)
    ps.append(Pairing("P7", "zstd_enc_slots", x, y, [("cj_debug_zstd_enc_slot_budget", SLOTS * ZSTD_ENC_SLOT)], (_ceil(x.n, SLOTS), _ceil(y.n, SLOTS))))
    x, y = dict_compress(512, 300, 15000), dict_compress(12, 700, 16000)
    ps.append(Pairing("P8", "dict_stage", x, y, [("cj_debug_dict_stage_budget", SLOTS * DICT_SLOT)], (_ceil(x.n, SLOTS), _ceil(y.n, SLOTS))))
    _cache["pairings"] = {p.name: p for p in ps}
    return _cache["pairings"]
