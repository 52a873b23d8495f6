"""The one harness of the device-resident batch tests: inputs packed at every misalignment, output slots with guard bytes
around them, one guarded run on an engine, and the checks behind it.  It knows no format and names no batch entry — the caller passes the
call — and it talks to an ENGINE OBJECT only (alloc / free / h2d / d2h / memset / sync), so tests/test_device_batch_model.py runs all of
it on a stand-in without a GPU.  Only numpy and the standard library are imported here: the torch child scripts import this module, and
they import torch before cramjam_amd on purpose (tests/device_api_child.py says why).

What every run gets: the whole output filled with 0xA5 before the call, the result row filled with 0x5A5A5A5A5A5A5A5A (a result that is
never written reads back as that, never as an expected 0), every buffer freed in `finally`, and a device error ends the session
(pytest.exit: no later test starts another GPU call).  What stays the caller's choice: the output slots' misalignment, whether
[result, cap) must stay untouched, and `written` for a refused chunk that may write inside its slot."""
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


# ---- children ------------------------------------------------------------------------------------------------------------------------------------
def run_child(script, marker, timeout, *args):
    """one fresh Python child on `script`: it must exit 0 and print `marker`"""
    r = subprocess.run([sys.executable, script] + list(args), capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and marker in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    return r
