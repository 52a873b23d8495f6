"""what the Blosc tests share: the fixtures of tests/golden/golden_blosc.json + .bin (valid chunks, malformed ones rebuilt from their
mutation specs) and the host build of the chunk grammar"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import blosc_model as M
import device_batch as DB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_doc = None


def doc():
    global _doc
    if _doc is None:
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosc.json")) as f:
            _doc = json.load(f)
        with open(os.path.join(ROOT, "tests", "golden", "golden_blosc.bin"), "rb") as f:
            blob = f.read()
        for i, v in enumerate(_doc["valid"]):
            v["name"] = M.name_of(v["recipe"], i)
            v["bytes"] = blob[v["at"]:v["at"] + v["len"]]
        for m in _doc["malformed"]:
            m["bytes"] = M.mutate(_doc["valid"][m["base"]]["bytes"], m["mutation"])
    return _doc


def valid(supported=True):
    return [v for v in doc()["valid"] if v["supported"] == supported]


def malformed():
    return doc()["malformed"]


def raw_of(v):
    r = v["recipe"]
    return M.make_input(r["kind"], r["size"], r["seed"])


_sim = None


def grammar_sim():
    """blosc_grammar.hpp for the host under ASan + UBSan, loaded in a child (the sanitizer runtime has to come first): see sim_child"""
    global _sim
    if _sim is None:
        so = os.path.join(ROOT, "tests", "hostsim", "libsim_blosc_grammar.so")
        src = os.path.join(ROOT, "tests", "hostsim", "sim_blosc_grammar.cpp")
        hdr = os.path.join(ROOT, "cramjam_amd", "csrc", "blosc_grammar.hpp")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, src])
        L = C.CDLL(so)
        L.sim_blosc_walk.restype = C.c_longlong
        L.sim_blosc_walk.argtypes = [C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p]
        L.sim_blosc_tr8.restype = C.c_ulonglong
        L.sim_blosc_tr8.argtypes = [C.c_ulonglong]
        L.sim_blosc_block_mode.restype = C.c_uint
        L.sim_blosc_block_mode.argtypes = [C.c_uint] * 3
        L.sim_blosc_layout.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_void_p]
        _sim = L
    return _sim


def sim_walk(L, chunk):
    """(code, header tuple, stream rows) — the chunk sits in an exact-size heap copy, so that a sanitizer sees any read past it"""
    buf = (C.c_ubyte * max(len(chunk), 1)).from_buffer_copy(chunk if chunk else b"\0")
    hdr = (C.c_uint * 8)()
    cap = 1 << 16
    rows = (C.c_uint * (6 * cap))()
    n = C.c_ulonglong(0)
    code = L.sim_blosc_walk(buf, len(chunk), hdr, rows, cap, C.byref(n))
    k = min(n.value, cap)
    return code, tuple(hdr), [tuple(rows[6 * i:6 * i + 6]) for i in range(k)]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def pack(chunks):
    """the chunks in one array, 16-byte aligned with a gap behind each: (blob, offsets, lengths)"""
    return DB.pack(chunks, mis=0)


def device_batch(e, N, chunks, caps, slots, flags, guard=0):
    """cj_blosc_batch_device (decode) in the harness's guarded run (tests/device_batch.py); slot i lies `guard` bytes behind slot
    i - 1's end, the whole output is filled with 0xA5 first: (results, the output bytes, the slots' offsets)"""
    blob, off, ln = pack(chunks)
    ooff, total = DB.out_slots(caps, guard=guard, slots=slots, tail=max(guard, 64) - guard)
    call = lambda i, o, l, out, oo, oc, r: N.check(N.lib().cj_blosc_batch_device(e.h, 0, i, o, l, out, oo, oc, r, len(chunks), None, flags, None))
    return DB.run(e, call, blob, off, ln, ooff, caps, total) + (ooff,)
