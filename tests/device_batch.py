"""The one harness of the device-resident batch tests: inputs packed at every misalignment, output slots with guard bytes
around them, one guarded run on an engine, and the checks behind it.  It knows no format and names no batch entry — the caller passes the
call — and it talks to an ENGINE OBJECT only (alloc / free / h2d / d2h / memset / sync), so tests/test_device_batch_model.py runs all of
it on a stand-in without a GPU.  Only numpy and the standard library are imported here: the torch child scripts import this module, and
they import torch before cramjam_amd on purpose (tests/device_api_child.py says why).

What every run gets: the whole output filled with 0xA5 before the call, the result row filled with 0x5A5A5A5A5A5A5A5A (a result that is
never written reads back as that, never as an expected 0), every buffer freed in `finally`, and a device error ends the session
(pytest.exit: no later test starts another GPU call).  What stays the caller's choice: the output slots' misalignment, whether
[result, cap) must stay untouched, and `written` for a refused chunk that may write inside its slot.

The far placement (far_layout / far_buffers / run_far, below) puts a case list around 2^31 and 2^32 of two allocations made once per
module: 6.06 GiB each, a peak of about 12.2 GiB of device memory (of the MI355X's 288 GB)."""
import contextlib
import subprocess
import sys

import numpy as np

G = 64                                   # guard bytes on both sides of every output slot
FILL = 0xA5                              # every output byte before the call
UNWRITTEN = 0x5A5A5A5A5A5A5A5A           # every result before the call


def in_mis(i): return (5 * i) % 16       # inputs: all sixteen residues over sixteen chunks in a row
def out_mis(i): return (7 * i) % 16      # output slots, where a file misaligns them too


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------
def pack(chunks, after=None, mis=in_mis, gap=16, dtype=np.uint64):
    """the chunks in one zeroed blob: chunk i at misalignment mis(i) (mis=0: none) behind a 16-byte boundary, `gap` bytes and more of
    zeros behind it.  after[i]: bytes packed right behind chunk i inside its own slot, not counted in its length — what a read past the
    input's end sees.  Returns (blob, off, lens), the last two as `dtype` (torch takes int64)."""
    off, run = np.zeros(len(chunks), np.uint64), 0
    tails = after if after is not None else [b""] * len(chunks)
    for i, (c, a) in enumerate(zip(chunks, tails)):
        m = mis(i) if mis else 0
        off[i] = run + m; run += (m + len(c) + len(a) + 15) // 16 * 16 + gap
    blob = np.zeros(run + 64, np.uint8)
    for o, c, a in zip(off, chunks, tails):
        b = bytes(c) + bytes(a)
        blob[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    return blob, off.astype(dtype), np.array([len(c) for c in chunks], dtype)


def out_slots(caps, guard=G, mis=None, slots=None, tail=64):
    """slot i lies `guard` bytes (+ mis(i)) behind slot i - 1's end; slots: the slots' sizes where they differ from the capacities;
    `tail` bytes behind the last guard.  Returns (ooff, total)."""
    ooff, run = [], guard
    for i, s in enumerate(caps if slots is None else slots):
        run += mis(i) if mis else 0
        ooff.append(run); run += int(s) + guard
    return np.array(ooff, np.uint64), run + tail


def untouched(ooff, want, total, written=None, sized=False):
    """the mask of the output bytes that must still be FILL after the call: all but [0, result) of an accepted chunk.  A refused chunk
    clears nothing, unless the caller says how much of its own slot it may have written before it found the stream bad: [0, written[i])
    (pass the capacities for "anywhere inside its slot").  sized (True, or per chunk): a size query has no output, nothing is cleared."""
    keep = np.ones(total, bool)
    for i, (lo, r) in enumerate(zip(ooff, want)):
        if sized if isinstance(sized, bool) else sized[i]:
            continue
        used = r if r >= 0 else (0 if written is None else written[i])
        keep[int(lo):int(lo) + int(used)] = False
    return keep


# ---- one run -----------------------------------------------------------------------------------------------------------------------------------
class _Batch:
    """what a run hands its caller: args = (d_in, in_off, in_len, d_out, out_off, out_cap, result), d_dict, and further buffers and rows"""

    def __init__(self, eng, n):
        self.eng, self.n, self._live = eng, n, []

    def buffer(self, nbytes, fill=None):
        p = self.eng.alloc(nbytes)
        self._live.append(p)
        if fill is not None:
            self.eng.memset(p, fill, nbytes)
        return p

    def rows(self, *arrays):
        """one more allocation of len(arrays) rows of n 64-bit words each, uploaded: their device pointers"""
        p = self.buffer(8 * self.n * len(arrays))
        self.eng.h2d(p, np.concatenate([np.asarray(a).astype(np.uint64) for a in arrays]))
        return [p + 8 * self.n * k for k in range(len(arrays))]

    def result_row(self):
        return self.rows(np.full(self.n, UNWRITTEN, np.uint64))[0]

    def output(self, caps):
        """a second guarded output, filled: (its base, out_off row, out_cap row, result row, the slots' offsets as ints, its size)"""
        ooff, total = out_slots(caps)
        return (self.buffer(total, FILL), *self.rows(ooff, caps), self.result_row(), [int(o) for o in ooff], total)

    def read_row(self, p):
        return self.eng.d2h(p, 8 * self.n, "int64")

    def read(self, with_input=False):
        """wait for the engine, then (results, output[, the input blob as it is now])"""
        self.eng.sync()
        got = self.read_row(self.args[6]), self.eng.d2h(self.args[3], self.total)
        return got + (self.eng.d2h(self.args[0], self.in_bytes),) if with_input else got

    def free(self):
        while self._live:
            self.eng.free(self._live.pop())


def _device_error():
    N = sys.modules.get("cramjam_amd._native")         # (not imported from here; a stand-in engine raises none of these)
    return N.EngineError if N is not None else ()


@contextlib.contextmanager
def device_batch(eng, blob, off, lens, ooff, caps, total, dictionary=None, fill=FILL, what=None):
    """allocate, upload, fill the output with `fill` and the results with UNWRITTEN, wait; the caller makes its call(s) on b.args and
    reads with b.read(); everything is freed whatever happens.  dictionary: uploaded 3 bytes off a granule, b.d_dict points at it."""
    b = _Batch(eng, len(off))
    try:
        b.in_bytes, b.total = blob.nbytes, total
        d_in = b.buffer(blob.nbytes)
        eng.h2d(d_in, blob)
        d_out = b.buffer(total, fill)
        m = b.rows(off, lens, ooff, caps, np.full(b.n, UNWRITTEN, np.uint64))
        b.args = (d_in, m[0], m[1], d_out, m[2], m[3], m[4])
        b.d_dict = None
        if dictionary is not None:
            b.d_dict = b.buffer(len(dictionary) + 32) + 3
            if len(dictionary):
                eng.h2d(b.d_dict, np.frombuffer(dictionary, np.uint8))
        eng.sync()
        yield b
    except _device_error() as ex:                      # a call or a copy failed on the device: no later test of the session starts another
        import pytest
        pytest.exit("device error in %r: %s" % (what, ex), 1)
    finally:
        b.free()


def run(eng, call, blob, off, lens, ooff, caps, total, dictionary=None, with_input=False, fill=FILL, what=None):
    """one call(d_in, in_off, in_len, d_out, out_off, out_cap, result[, d_dict]) in a device_batch: what b.read(with_input) returns"""
    with device_batch(eng, blob, off, lens, ooff, caps, total, dictionary, fill, what) as b:
        call(*(b.args + ((b.d_dict,) if dictionary is not None else ())))
        return b.read(with_input)


def run_chunks(eng, call, chunks, caps, out_mis=None, dictionary=None):
    """pack() + out_slots() + run() for plain lists of chunks and capacities: (results, output, the slots' offsets as ints)"""
    blob, off, lens = pack(chunks)
    ooff, total = out_slots(caps, mis=out_mis)
    res, out = run(eng, call, blob, off, lens, ooff, caps, total, dictionary)
    return res, out, [int(o) for o in ooff]


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------------
def guards_intact(out, ooff, caps, guard=G, fill=FILL):
    """nothing outside the slots (what a chunk left inside its slot does not matter): the first offending chunk or None"""
    for i, (lo, cap) in enumerate(zip(ooff, caps)):
        lo, hi = int(lo), int(lo) + int(cap)
        if not ((out[lo - guard:lo] == fill).all() and (out[hi:hi + guard] == fill).all()):
            return i
    return None


def first_dirty(out, keep, ooff, fill=FILL):
    """None, or (chunk, offset within its slot, how many bytes changed) for the first byte of the mask that is no longer `fill`"""
    dirty = np.nonzero(out[keep] != fill)[0]
    if not len(dirty):
        return None
    at = int(np.nonzero(keep)[0][dirty[0]])
    i = max(int(np.searchsorted(np.asarray(ooff, np.uint64), at, side="right")) - 1, 0)
    return i, at - int(ooff[i]), len(dirty)


def check_mask(out, keep, ooff, tag, what="a byte outside [0, result) changed", fill=FILL):
    bad = first_dirty(out, keep, ooff, fill)
    assert bad is None, (what, bad[1], bad[2], tag(bad[0]))


def check_results(res, want, tag):
    bad = np.nonzero(np.asarray(res) != np.asarray(want, np.int64))[0]
    assert len(bad) == 0, (len(bad), [tag(int(i)) for i in bad[:6]])


# ---- lists of cases --------------------------------------------------------------------------------------------------------------------------------
# A case is a dict: `bytes` (the input), `cap`, `result` and `out` (the expected bytes; None: `sha`, their sha256); optional `after`
# (pack), `written` (untouched; without it a refused chunk may write anywhere inside its slot) and `sized` (a size query: no output).
# The far runner also takes result = None with `at_least` and `verify`: any result from at_least to cap whose bytes verify(bytes) accepts.
_packs, _slots = {}, {}


def case_pack(key, cases):
    """pack() of a case list, once per key"""
    if key not in _packs:
        _packs[key] = pack([c["bytes"] for c in cases], [c.get("after", b"") for c in cases])
    assert len(_packs[key][1]) == len(cases), ("one key, two case lists", key)
    return _packs[key]


def case_slots(key, cases):
    """once per key: (caps, ooff, total, keep, want) — out_slots() and untouched() of a case list"""
    if key not in _slots:
        caps, want = np.array([c["cap"] for c in cases], np.uint64), np.array([c["result"] for c in cases], np.int64)
        ooff, total = out_slots(caps)
        keep = untouched(ooff, want, total, written=[c.get("written", c["cap"]) for c in cases], sized=[bool(c.get("sized")) for c in cases])
        _slots[key] = caps, ooff, total, keep, want
    assert len(_slots[key][0]) == len(cases), ("one key, two case lists", key)
    return _slots[key]


def run_cases(eng, key, cases, call, tag, packed=None, more=0, dictionary=None, with_input=False, what="a byte outside [0, result) changed"):
    """one device batch over a case list (packed: a (blob, off) made elsewhere; more: bytes added to every in_len) held to every case's
    result — tag(i, got) names a failing case —, to the mask, to the expected bytes and, with_input, to an input blob read back unchanged.
    Returns (results, output, ooff)."""
    import hashlib
    blob, off = packed if packed is not None else case_pack(key, cases)[:2]
    caps, ooff, total, keep, want = case_slots(key, cases)
    lens = np.array([len(c["bytes"]) + more for c in cases], np.uint64)
    got = run(eng, call, blob, off, lens, ooff, caps, total, dictionary, with_input, what=key)
    res, out = got[:2]
    check_results(res, want, lambda i: tag(i, int(res[i])))
    check_mask(out, keep, ooff, lambda i: tag(i, int(res[i])), what)
    for i in np.nonzero(want > 0)[0]:
        c = cases[i]
        if c.get("sized"):
            continue
        b = out[int(ooff[i]):int(ooff[i]) + int(want[i])]
        assert (b.tobytes() == c["out"]) if c.get("out") is not None else (hashlib.sha256(bytes(b)).hexdigest() == c["sha"]), ("bytes", tag(i, int(res[i])))
    assert not with_input or (got[2] == blob).all(), ("the input was written", key)
    return res, out, ooff


# ---- the far placement -----------------------------------------------------------------------------------------------------------------------------
# A device entry addresses chunk i as in_base + in_off[i] and out_base + out_off[i] with 64-bit rows.  The far placement puts a case
# list around a LINE of `bits` bits (32 on the GPU, 20 on the CPU stand-in) inside two allocations made once per module, each of
# far_size(bits) = 2^(bits-1) + 2^bits + 2^(bits-6) bytes (bits = 32: 2 GiB + 4 GiB + 64 MiB = 6.06 GiB each, 12.2 GiB at the peak).
# THE INVARIANT: the base handed to the entry is allocation start + 2^(bits-1), so offsets -2^(bits-1) .. 2^bits + 2^(bits-6) are memory
# of the allocation; an address whose low `bits` bits were cut out of a 64-bit offset and zero-extended lies at o mod 2^bits, one that was
# sign-extended at o - 2^bits for o mod 2^bits >= 2^(bits-1): both inside the allocation for every byte of every slot.  So a kernel with
# such an address reads a decoy or writes a shadow window — an assertion here, never a GPU fault.  far_layout() asserts it byte by byte.
#
# The cases of a list are dealt round-robin over four places: A around 2^(bits-1) and B around 2^bits (in both the longest input, and
# the output slot with the largest positive result, has its first byte below the line and its last byte above it), C with its first
# slot exactly at 2^bits, D from 2^bits + 2^(bits-7) + 5.  B's straddling chunk occupies the byte at 2^bits where C's first slot
# begins, so one list is two calls of the entry: FAR_CALLS.  Inside a place the inputs keep pack()'s misalignments and gaps, the
# output slots out_slots()'s 64 guard bytes.  Only windows are ever filled, uploaded or read back.
PLACES = "ABCD"
FAR_CALLS = (("A", "B", "D"), ("C",))
FAR_MARGIN = 1 << 20                     # bytes of 0xA5 around a place's output slots (the stand-in passes a smaller one)


def far_size(bits):
    return (1 << (bits - 1)) + (1 << bits) + (1 << (bits - 6))


def far_pieces(lo, hi, bits):
    """[lo, hi) cut at the two lines: (a, b, where a lies with its low `bits` bits zero-extended, where sign-extended) per piece"""
    H, L = 1 << (bits - 1), 1 << bits
    cuts = sorted({lo, hi} | {x for x in (H, L) if lo < x < hi})
    for a, b in zip(cuts, cuts[1:]):
        z = a % L
        yield a, b, z, z - L if z >= H else z


def _shadows(lo, hi, bits):
    """the windows where a truncated address of a byte of [lo, hi) lies: (shadow lo, shadow hi, lo of the bytes it shadows, kind)"""
    for a, b, z, s in far_pieces(lo, hi, bits):
        if z == s != a:
            yield z, z + b - a, a, "zero/sign"
        else:
            if z != a:
                yield z, z + b - a, a, "zero"
            if s != a:
                yield s, s + b - a, a, "sign"


def _straddle(off, sizes, align=1):
    """(which slot, how many of its bytes lie below the line): the largest slot, cut near its middle (align: so that the place begins
    on a multiple of it); None when no slot has two bytes"""
    s = int(np.argmax(sizes))
    n = int(sizes[s])
    if n < 2:
        return None
    ks = [k for k in range(1, n) if (int(off[s]) + k) % align == 0] or [n // 2]
    return s, min(ks, key=lambda k: abs(k - n // 2))


def _origin(place, bits, off, sizes, first, align=1):
    """where a place's run begins so that A and B straddle their line, C's slot 0 (`first` bytes into the run) lies at 2^bits, D's at 2^bits + 2^(bits-7) + 5"""
    H, L = 1 << (bits - 1), 1 << bits
    if place in "AB":
        line, st = (H if place == "A" else L), _straddle(off, sizes, align)
        return line - int(off[st[0]]) - st[1] if st else line - first - 16
    return (L if place == "C" else L + (1 << (bits - 7)) + 5) - first


def _view(real, decoy, o, bits, kind):
    """what a read of len(real) bytes at offset o sees when every byte's address is truncated in the `kind` way"""
    out = bytearray(real)
    for a, b, z, s in far_pieces(o, o + len(real), bits):
        if (z if kind == "zero" else s) != a:
            out[a - o:b - o] = decoy[a - o:b - o]
    return bytes(out)


class FarLayout:
    """one call of a far list: idx (the cases of this call, as indices of the list), the four rows in_off / in_len / out_off / out_cap
    relative to the base, want, the input windows [(address, bytes)] with the decoys among them, the output windows [(address, size)]
    with the shadow windows among them, out_shadows [(lo, hi, chunk, kind)], decoys {chunk: (case, bytes)}, places, straddlers"""


_far = {}


def far_layout(key, cases, bits, places, margin=FAR_MARGIN):
    """the layout of the cases that fall into `places`, once per (key, places), with the invariant asserted"""
    if (key, bits, places) in _far:
        assert _far[(key, bits, places)].n_all == len(cases), ("one key, two case lists", key)
        return _far[(key, bits, places)]
    H, L, end = 1 << (bits - 1), 1 << bits, far_size(bits) - (1 << (bits - 1))
    F = FarLayout()
    F.n_all, F.bits, F.places = len(cases), bits, places
    F.idx = [i for i in range(len(cases)) if PLACES[i % 4] in places]
    n = len(F.idx)
    F.in_off, F.out_off = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    F.in_len = np.array([len(cases[i]["bytes"]) for i in F.idx], np.uint64)
    F.caps = np.array([cases[i]["cap"] for i in F.idx], np.uint64)
    F.unknown = [k for k, i in enumerate(F.idx) if cases[i]["result"] is None]          # `verify` cases: at_least <= result <= cap, the bytes to verify()
    F.want = np.array([cases[i]["at_least"] if cases[i]["result"] is None else cases[i]["result"] for i in F.idx], np.int64)
    F.in_windows, F.out_places, F.straddlers = [], [], {}
    for p in places:
        loc = [k for k, i in enumerate(F.idx) if PLACES[i % 4] == p]
        cs = [cases[F.idx[k]] for k in loc]
        blob, off, lens = pack([c["bytes"] for c in cs], [c.get("after", b"") for c in cs])
        org = _origin(p, bits, off, lens, 0, 16)
        F.in_off[loc] = off + np.uint64(org)
        F.in_windows.append((org - G, np.concatenate([np.zeros(G, np.uint8), blob])))
        ooff, total = out_slots(F.caps[loc])
        real = [0 if c.get("sized") else c["at_least"] if c["result"] is None else max(int(c["result"]), 0) for c in cs]
        oo = _origin(p, bits, ooff, real if max(real) >= 2 else F.caps[loc], G)
        F.out_off[loc] = ooff + np.uint64(oo)
        F.out_places.append((oo - margin, total + 2 * margin, loc, ooff + np.uint64(margin)))
        line = H if p == "A" else L                  # (first byte below the line, last byte on or above it)
        F.straddlers[p] = ([k for k in loc if int(F.in_off[k]) < line < int(F.in_off[k]) + int(F.in_len[k])],
                           [k for k in loc if not cases[F.idx[k]].get("sized") and int(F.out_off[k]) < line < int(F.out_off[k]) + int(F.want[k])])
    # the decoys: behind every truncated address of an input byte lie the bytes of another case of the list
    F.decoys, F.in_shadows = {}, []
    for k, i in enumerate(F.idx):
        o, real = int(F.in_off[k]), cases[i]["bytes"]
        sh = list(_shadows(o, o + len(real), bits))
        if not sh:
            continue
        moved = [kind for kind in ("zero", "sign") if any(s[3] in (kind, "zero/sign") for s in sh)]
        differs = lambda decoy: len(decoy) == len(real) and all(_view(real, decoy, o, bits, kind) != real for kind in moved)
        for j, tail in [((i + d) % len(cases), t) for t in (False, True) for d in range(1, len(cases))]:
            other = cases[j]["bytes"]              # the next case of the list whose head differs (tiled when it is shorter); cuts of one stream: whose tail does
            decoy = other[-len(real):] if tail else (other * (len(real) // max(len(other), 1) + 1))[:len(real)]
            if differs(decoy):
                break
        else:
            raise AssertionError(("no other case of the list differs from this one", key, i))
        F.decoys[k] = (j, decoy)
        for lo, hi, a, kind in sh:
            F.in_shadows.append((lo, hi, k, kind))
            F.in_windows.append((lo, np.frombuffer(decoy[a - o:a - o + hi - lo], np.uint8)))
    # the shadows of every output slot and its guards, merged into windows
    F.out_shadows = [(lo, hi, k, kind) for k in range(n) for lo, hi, _, kind in _shadows(int(F.out_off[k]) - G, int(F.out_off[k]) + int(F.caps[k]) + G, bits)]
    F.shadow_windows = []
    for lo, hi in sorted((lo, hi) for lo, hi, _, _ in F.out_shadows):
        if F.shadow_windows and lo <= F.shadow_windows[-1][1] + 4096:
            F.shadow_windows[-1][1] = max(hi, F.shadow_windows[-1][1])
        else:
            F.shadow_windows.append([lo, hi])
    # the invariant, and that no window lies on another
    for k in range(n):
        for lo, hi in ((int(F.in_off[k]), int(F.in_off[k]) + int(F.in_len[k])), (int(F.out_off[k]) - G, int(F.out_off[k]) + int(F.caps[k]) + G)):
            assert 0 <= lo <= hi <= end, ("a slot outside the allocation", key, F.idx[k])
            for a, b, z, s in far_pieces(lo, hi, bits):                   # (every byte of a piece moves by the same distance)
                assert -H <= min(z, s) and max(z, s) + b - a <= end, ("a truncated address outside the allocation", key, F.idx[k])
    for lo, hi, _, _ in F.in_shadows + F.out_shadows:
        assert -H <= lo <= hi <= end, ("a shadow outside the allocation", key)
    ins = sorted((a, a + len(b)) for a, b in F.in_windows if len(b))
    assert all(x[1] <= y[0] for x, y in zip(ins, ins[1:])) and -H <= ins[0][0] and ins[-1][1] <= end, ("two input windows overlap", key, ins)
    outs = sorted([(a, a + sz) for a, sz, _, _ in F.out_places] + [tuple(w) for w in F.shadow_windows])
    assert all(x[1] <= y[0] for x, y in zip(outs, outs[1:])) and -H <= outs[0][0] and outs[-1][1] <= end, ("two output windows overlap", key, outs)
    _far[(key, bits, places)] = F
    return F


class Far:
    """the two allocations of a module: d_in and d_out are the BASES (allocation start + 2^(bits-1))"""


@contextlib.contextmanager
def far_buffers(eng, bits=32):
    """the two far allocations, freed whatever happens.  On a card that cannot hold them (12.2 GiB for bits = 32) the tests that ask
    for them are skipped — decided here, before any call runs under device_batch()'s "a device error ends the session"."""
    f, live = Far(), []
    f.bits, f.size = bits, far_size(bits)
    try:
        try:
            for _ in range(2):
                live.append(eng.alloc(f.size))
        except _device_error() as ex:
            import pytest
            pytest.skip("the far placement needs two device allocations of %d bytes (%.2f GiB each): %s" % (f.size, f.size / 2.0 ** 30, ex))
        f.d_in, f.d_out = (p + (1 << (bits - 1)) for p in live)
        yield f
    finally:
        for p in live:
            eng.free(p)


def _named_kind(hits, clean_sign_only):
    """one word for a list of dirty kinds: a shadow that only a sign extension reaches decides for it, one that both reach is a zero
    extension when a sign-only shadow that a sign extension would have hit stayed clean"""
    if "sign" in hits:
        return "sign"
    return "zero" if "zero" in hits or clean_sign_only else "zero/sign"


def run_far(eng, far, key, cases, call, tag, dictionary=None, margin=FAR_MARGIN, calls=FAR_CALLS):
    """a case list at the far places: per FAR_CALLS one call(idx, d_in, in_off, in_len, d_out, out_off, out_cap, result[, d_dict]) on the
    module's two allocations (idx: the cases of this call, as indices of the list), held to every case's result and bytes, to [result, cap) and the guards and margin around every slot, to
    every shadow window still 0xA5, and to input windows read back unchanged.  tag(i, got) names case i of the list; calls: the
    places of each call, where a caller wants other ones than FAR_CALLS."""
    import hashlib
    bits = far.bits
    for places in calls:
        F = far_layout(key, cases, bits, places, margin)
        n = len(F.idx)
        if not n:
            continue
        b = _Batch(eng, n)
        try:
            for a, data in F.in_windows:
                if len(data):
                    eng.h2d(far.d_in + a, data)
            for a, sz in [(a, sz) for a, sz, _, _ in F.out_places] + [(lo, hi - lo) for lo, hi in F.shadow_windows]:
                eng.memset(far.d_out + a, FILL, sz)
            m = b.rows(F.in_off, F.in_len, F.out_off, F.caps, np.full(n, UNWRITTEN, np.uint64))
            d_dict = None
            if dictionary is not None:
                d_dict = b.buffer(len(dictionary) + 32) + 3
                if len(dictionary):
                    eng.h2d(d_dict, np.frombuffer(dictionary, np.uint8))
            eng.sync()
            call(*((list(F.idx), far.d_in, m[0], m[1], far.d_out, m[2], m[3], m[4]) + ((d_dict,) if dictionary is not None else ())))
            eng.sync()
            res = b.read_row(m[4])
            outs = [eng.d2h(far.d_out + a, sz) for a, sz, _, _ in F.out_places]
            shadows = [(lo, eng.d2h(far.d_out + lo, hi - lo)) for lo, hi in F.shadow_windows]
            back = [eng.d2h(far.d_in + a, len(data)) for a, data in F.in_windows]
        except _device_error() as ex:
            import pytest
            pytest.exit("device error in %r: %s" % (key, ex), 1)
        finally:
            b.free()
        name = lambda k: tag(F.idx[k], int(res[k]))
        want = F.want.copy()
        for k in F.unknown:                                  # (an encoder without a byte-exact model: any length its own verify() accepts)
            assert F.want[k] <= res[k] <= F.caps[k], ("result", name(k))
            want[k] = res[k]
        # a write at a truncated out_off: the most telling failure first
        dirty = []
        for lo, hi, k, kind in F.out_shadows:
            base, w = next((a, w) for a, w in shadows if a <= lo and hi <= a + len(w))
            dirty.append((w[lo - base:hi - base] != FILL).any())
        hits = [(k, kind) for (_, _, k, kind), d in zip(F.out_shadows, dirty) if d]
        if hits:
            wrote = lambda k: want[k] > 0 and not cases[F.idx[k]].get("sized")
            clean = any(kind == "sign" and wrote(k) and not d for (_, _, k, kind), d in zip(F.out_shadows, dirty))
            raise AssertionError("chunk %r written at its offset truncated to %d bits (%s)" % (name(hits[0][0]), bits, _named_kind([h[1] for h in hits], clean)))
        # results and bytes; a chunk that came out as its decoy was read at a truncated in_off
        got = {}
        for (a, sz, loc, _), out in zip(F.out_places, outs):
            for k in loc:
                lo = int(F.out_off[k]) - a
                got[k] = out[lo:lo + max(int(want[k]), 0)]
        reads = {}
        for k, (j, decoy) in F.decoys.items():
            o, real = int(F.in_off[k]), cases[F.idx[k]]["bytes"]
            reads[k] = {kind: _view(real, decoy, o, bits, kind) for kind in ("zero", "sign")}
        copied = [[kind for kind, v in reads[k].items() if v != cases[F.idx[k]]["bytes"] and got[k].tobytes() == v] for k in sorted(reads)]
        if any(copied):
            k = next(k for k, c in zip(sorted(reads), copied) if c)
            kinds = ["/".join(c) for c in copied if c]
            sign_only = any(reads[k]["sign"] != reads[k]["zero"] and not c for k, c in zip(sorted(reads), copied))
            raise AssertionError("chunk %r read at its offset truncated to %d bits (%s)" % (name(k), bits, _named_kind(kinds, sign_only)))
        note = lambda k: name(k) + (("in place", PLACES[F.idx[k] % 4]) + (("its truncated in_off holds case", F.decoys[k][0]) if k in F.decoys else ()),)
        bad = np.nonzero(res != want)[0]
        assert len(bad) == 0, (len(bad), [note(int(k)) for k in bad[:6]])
        for k in np.nonzero(want > 0)[0]:
            c = cases[F.idx[k]]
            if c.get("verify"):
                c["verify"](got[k].tobytes())
            elif not c.get("sized"):
                assert (got[k].tobytes() == c["out"]) if c.get("out") is not None else (hashlib.sha256(bytes(got[k])).hexdigest() == c["sha"]), ("bytes", note(int(k)))
        for (a, sz, loc, at), out in zip(F.out_places, outs):
            cs = [cases[F.idx[k]] for k in loc]
            keep = untouched(at, want[loc], sz, written=[c.get("written", c["cap"]) for c in cs], sized=[bool(c.get("sized")) for c in cs])
            check_mask(out, keep, at, lambda q: name(loc[q]), "a guard byte or a byte outside [0, result) changed")
        for (a, data), now in zip(F.in_windows, back):
            assert (now == data).all(), ("the input was written", key, a)


# ---- children ------------------------------------------------------------------------------------------------------------------------------------
def run_child(script, marker, timeout, *args):
    """one fresh Python child on `script`: it must exit 0 and print `marker`"""
    r = subprocess.run([sys.executable, script] + list(args), capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and marker in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    return r
