"""The bounds-checked stand-ins of tests/hostsim/sim_wave.hpp, which every host build of a wave decoder is written over, held
themselves (tests/hostsim/sim_standins.cpp): each checked accessor at the last legal position, where it must move the right bytes, and
one byte beyond at each end, where it must answer SIM_BOUNDS; the register window's precondition; the copies' source rules.  No GPU."""
import ctypes as C

import pytest

from hostsim_build import build_sim

SIM_BOUNDS = -9999
REC, REC_N, IN, IN_N, SRC2, SRC2_N, OUT, OUT_N, LDS, LDS_N = 16, 32, 64, 40, 104, 24, 160, 48, 224, 32
(IN_LD8, IN_LD32, OUT_LD8, OUT_RD32, OUT_ST8, OUT_ST32, SLOT_ST8, LDS_LD, LDS_LD8, LDS_ADD, LDS_XOR, LDS_OR, COPY, MATCH, PUT, FLUSH,
 FETCH32, OPEN, LANE_U32, LANE_U64, EXCL_ADD, REC_LD) = range(22)
FRESH = bytes(range(256))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    L = C.CDLL(build_sim("sim_standins.cpp", str(tmp_path_factory.mktemp("standins") / "libsim_standins.so")))
    L.standin.restype = C.c_longlong
    L.standin.argtypes = [C.c_int, C.c_long, C.c_long, C.c_long]

    def run(op, a=0, b=0, c=0):
        r = L.standin(op, a, b, c)
        buf = C.create_string_buffer(256)
        L.standin_arena(buf)
        return r, buf.raw
    return run


def le32(b, at):
    return int.from_bytes(b[at:at + 4], "little")


@pytest.mark.parametrize("op,base,size,width", [(IN_LD8, IN, IN_N, 1), (IN_LD32, IN, IN_N, 4), (OUT_LD8, OUT, OUT_N, 1), (OUT_RD32, OUT, OUT_N, 4),
                                                (LDS_LD, LDS, LDS_N, 4), (LDS_LD8, LDS, LDS_N, 1)])
def test_loads_at_both_edges(S, op, base, size, width):
    for at in (0, size - width):
        r, arena = S(op, at)
        assert r == int.from_bytes(FRESH[base + at:base + at + width], "little") and arena == FRESH
    for at in (-1, size - width + 1):
        assert S(op, at) == (SIM_BOUNDS, FRESH)


@pytest.mark.parametrize("op,base,size,width,fn", [(OUT_ST8, OUT, OUT_N, 1, lambda old, v: v), (OUT_ST32, OUT, OUT_N, 4, lambda old, v: v),
                                                   (SLOT_ST8, SRC2, SRC2_N, 1, lambda old, v: v), (LDS_ADD, LDS, LDS_N, 4, lambda old, v: (old + v) & 0xFFFFFFFF),
                                                   (LDS_XOR, LDS, LDS_N, 4, lambda old, v: old ^ v), (LDS_OR, LDS, LDS_N, 4, lambda old, v: old | v)])
def test_stores_at_both_edges(S, op, base, size, width, fn):
    v = 0xC3D2E1F0 if width == 4 else 0x5C
    for at in (0, size - width):
        r, arena = S(op, at, v)
        want = bytearray(FRESH)
        want[base + at:base + at + width] = fn(le32(FRESH, base + at), v).to_bytes(4, "little")[:width]
        assert r == 0 and arena == bytes(want), (op, at)
    for at in (-1, size - width + 1):
        assert S(op, at, v) == (SIM_BOUNDS, FRESH), (op, at)


def test_register_window(S):
    # fetch32 needs pos - wpos <= 507: the last legal distance, then one more.  Bytes outside the stream [IN, IN + IN_N) read as 0xEE
    assert S(FETCH32, IN, IN + 4)[0] == le32(FRESH, IN + 4)
    assert S(FETCH32, IN, IN + 507)[0] == 0xEEEEEEEE
    assert S(FETCH32, IN, IN + 508)[0] == SIM_BOUNDS
    assert S(FETCH32, IN, IN + IN_N - 2)[0] == le32(FRESH[:IN + IN_N] + b"\xee\xee", IN + IN_N - 2)
    assert S(FETCH32, IN - 4, IN - 2)[0] == le32(b"\xee" * IN + FRESH[IN:], IN - 2)      # (below a misaligned stream's first byte)
    # window_open(): base = the dword boundary at or below the stream, iend and the anchor relative to it
    for mis in (0, 1, 3):
        r = S(OPEN, mis, 9)[0]
        assert (r & 0xFF, (r >> 8) & 0xFF, (r >> 16) & 0xFFFF, r >> 32) == (mis, IN, mis + 9, 0)


def test_lane_values(S):
    assert S(PUT, 63, 0x1AB)[0] == 0xAB and S(PUT, 64, 1)[0] == SIM_BOUNDS
    r, arena = S(FLUSH, OUT_N - 64 + 16, 0)                    # (n == 0 stores nothing, wherever it points inside the output)
    assert r == 0 and arena == FRESH
    r, arena = S(FLUSH, 0, OUT_N)
    assert r == 0 and arena == FRESH[:OUT] + bytes(k ^ 0x5A for k in range(OUT_N)) + FRESH[OUT + OUT_N:]
    assert S(FLUSH, 1, OUT_N) == (SIM_BOUNDS, FRESH) and S(FLUSH, -1, 4) == (SIM_BOUNDS, FRESH) and S(FLUSH, 0, 65)[0] == SIM_BOUNDS
    assert S(LANE_U32, 63)[0] == 7 and S(LANE_U32, 64)[0] == SIM_BOUNDS
    assert S(LANE_U64, 63)[0] == 7 and S(LANE_U64, 64)[0] == SIM_BOUNDS
    for lane in (0, 1, 63):
        assert S(EXCL_ADD, lane)[0] == (2080 << 32) | (lane * (lane + 1) // 2)


def test_record_loads(S):
    # rec_ld(slot, i): record i of 16 bytes wholly inside the record range
    assert S(REC_LD, 0, 0) == (le32(FRESH, REC + 12), FRESH) and S(REC_LD, 0, 1) == (le32(FRESH, REC + 28), FRESH)
    assert S(REC_LD, 0, 2)[0] == SIM_BOUNDS and S(REC_LD, 1, 1)[0] == SIM_BOUNDS and S(REC_LD, -1, 0)[0] == SIM_BOUNDS
    assert S(REC_LD, -16, 1)[0] == le32(FRESH, REC + 12) and S(REC_LD, -16, 0)[0] == SIM_BOUNDS


def test_wave_copy_sources_and_destination(S):
    def moved(dst, src, n):
        return FRESH[:OUT + dst] + FRESH[src:src + n] + FRESH[OUT + dst + n:]
    assert S(COPY, 0, IN, IN_N) == (0, moved(0, IN, IN_N))                                   # the whole stream
    assert S(COPY, OUT_N - SRC2_N, SRC2, SRC2_N) == (0, moved(OUT_N - SRC2_N, SRC2, SRC2_N))   # the whole second range, to the last byte of the output
    assert S(COPY, 0, IN - 1, 4) == (SIM_BOUNDS, FRESH) and S(COPY, 0, SRC2 + SRC2_N - 3, 4) == (SIM_BOUNDS, FRESH)
    assert S(COPY, 0, IN + IN_N - 2, 4) == (SIM_BOUNDS, FRESH)                               # a run across the stream's end into the second range
    assert S(COPY, -1, IN, 4) == (SIM_BOUNDS, FRESH) and S(COPY, OUT_N - 3, IN, 4) == (SIM_BOUNDS, FRESH)
    assert S(COPY, 0, OUT, 4) == (SIM_BOUNDS, FRESH)                                         # the output is no source
    assert S(COPY, -100, 0, 0) == (0, FRESH)                                                 # nothing to move: no access


def test_wave_match_copy(S):
    r, arena = S(MATCH, 3, 3, OUT_N - 3)                       # from the output's first byte to its last, overlapping: period 3
    assert r == 0 and arena == FRESH[:OUT] + bytes(FRESH[OUT + k % 3] for k in range(OUT_N)) + FRESH[OUT + OUT_N:]
    assert S(MATCH, 3, 0, 4) == (SIM_BOUNDS, FRESH)            # distance 0
    assert S(MATCH, 3, 0, 0) == (SIM_BOUNDS, FRESH)            # ... of an empty match too
    assert S(MATCH, 3, 4, 4) == (SIM_BOUNDS, FRESH)            # dst - d one byte below the output
    assert S(MATCH, 3, 3, OUT_N - 2) == (SIM_BOUNDS, FRESH)    # one byte beyond its end
    assert S(MATCH, -1, 1, 1) == (SIM_BOUNDS, FRESH)
