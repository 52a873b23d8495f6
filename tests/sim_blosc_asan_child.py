"""child of tests/test_blosc_model.py: walks every fixture through blosc_grammar.hpp built with -fsanitize=address,undefined.
Every chunk is copied into a malloc block of exactly its size first, so a read outside [chunk, chunk + len) aborts the process."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blosc_cases as K  # noqa: E402


def main():
    so = sys.argv[1]
    L = C.CDLL(so)
    L.sim_blosc_walk.restype = C.c_longlong
    L.sim_blosc_walk.argtypes = [C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p]
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    hdr = (C.c_uint * 8)()
    rows = (C.c_uint * (6 * 65536))()
    n = C.c_ulonglong(0)
    count = 0
    for e in K.doc()["valid"] + K.doc()["malformed"]:
        b = e["bytes"]
        p = libc.malloc(max(len(b), 1))
        C.memmove(p, b, len(b))
        L.sim_blosc_walk(p, len(b), hdr, rows, 65536, C.byref(n))
        libc.free(p)
        count += 1
    print("walked", count)


if __name__ == "__main__":
    main()
