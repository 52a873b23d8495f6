"""tests/device_batch.py on the CPU: the layouts as literal numbers, a well-behaved call, and one test per fault the harness exists to
catch — each asserting WHICH chunk and offset the failure names.  The engine is a stand-in over one bytearray; the "kernel" is a Python
function that copies every chunk that fits into its slot and refuses (-3) the others."""
import os

import numpy as np
import pytest

import device_batch as DB

LENS = (0, 1, 15, 16, 17, 33)
CAPS = (0, 1, 16, 16, 40, 16)                       # chunk 4 leaves [17, 40) behind its result; chunk 5 does not fit: refused
CHUNKS = [bytes(range(s, s + n)) for s, n in zip((1, 2, 10, 30, 50, 100), LENS)]        # (no byte is 0x00, 0xA5 or 0x5A)
WANT = [0, 1, 15, 16, 17, -3]
OOFF = [64, 128, 193, 273, 353, 457]                # 64 guard bytes in front of slot 0, capacity + 64 from slot to slot
tag = lambda i: ("chunk", i)


class Engine:
    """alloc / free / h2d / d2h / memset / sync over one address space; allocations 256 bytes apart so that an overrun lands in nobody's buffer"""

    def __init__(self):
        self.mem, self.live = bytearray(4096), {}

    def alloc(self, nbytes):
        p = len(self.mem)
        self.mem += bytes(-(-nbytes // 256) * 256 + 256)
        self.live[p] = nbytes
        return p

    def free(self, p):
        del self.live[p]

    def h2d(self, p, data):
        b = np.ascontiguousarray(data).tobytes()
        self.mem[p:p + len(b)] = b

    def d2h(self, p, nbytes, dtype="uint8"):
        return np.frombuffer(bytes(self.mem[p:p + nbytes]), dtype).copy()

    def memset(self, p, value, nbytes):
        self.mem[p:p + nbytes] = bytes([value]) * nbytes

    def sync(self):
        pass


def kernel(eng, n, fault=None, skip_result=()):
    def call(d_in, in_off, in_len, d_out, out_off, out_cap, result):
        row = lambda p: eng.d2h(p, 8 * n, "int64")
        for i, (o, ln, oo, cap) in enumerate(zip(row(in_off), row(in_len), row(out_off), row(out_cap))):
            if ln <= cap:
                eng.mem[d_out + oo:d_out + oo + ln] = eng.mem[d_in + o:d_in + o + ln]
            if i not in skip_result:
                eng.h2d(result + 8 * i, np.int64(ln if ln <= cap else -3))
        if fault:
            fault(eng.mem, d_in, d_out)
    return call


def one_run(fault=None, skip_result=(), mis=None):
    eng = Engine()
    blob, off, lens = DB.pack(CHUNKS)
    ooff, total = DB.out_slots(CAPS, mis=mis)
    res, out, back = DB.run(eng, kernel(eng, len(CHUNKS), fault, skip_result), blob, off, lens, ooff, CAPS, total, with_input=True)
    assert not eng.live
    return res, out, back, blob, ooff, total


# ---- layout ------------------------------------------------------------------------------------------------------------------------------------
def test_input_layout_is_these_numbers():
    blob, off, lens = DB.pack(CHUNKS)
    assert off.tolist() == [0, 21, 58, 111, 148, 201] and lens.tolist() == list(LENS) and blob.nbytes == 256 + 64
    assert [int(o) % 16 for o in off] == [0, 5, 10, 15, 4, 9]
    for o, c in zip(off, CHUNKS):
        assert blob[int(o):int(o) + len(c)].tobytes() == c
    assert int(blob.astype(np.int64).sum()) == sum(sum(c) for c in CHUNKS)          # zeros everywhere else
    blob, off, _ = DB.pack(CHUNKS, mis=0)                                           # the torch children's packing
    assert off.tolist() == [0, 16, 48, 80, 112, 160] and blob.nbytes == 224 + 64
    blob, off, _ = DB.pack(CHUNKS, mis=0, gap=32)
    assert off.tolist() == [0, 32, 80, 128, 176, 240] and blob.nbytes == 320 + 64


def test_input_layout_with_after_bytes():
    after = [b"", b"ab", b"", b"x" * 16, b"", b"zzz"]
    blob, off, lens = DB.pack(CHUNKS, after=after)
    assert off.tolist() == [0, 21, 58, 111, 164, 217] and lens.tolist() == list(LENS) and blob.nbytes == 272 + 64
    for o, c, a in zip(off, CHUNKS, after):
        assert blob[int(o):int(o) + len(c) + len(a) + 16].tobytes() == c + a + bytes(16)      # 16 zero bytes and more behind `after`


def test_every_promised_input_residue_occurs():
    _, off, _ = DB.pack([b"q" * (3 * i) for i in range(16)])
    assert sorted(int(o) % 16 for o in off) == list(range(16))
    ooff, _ = DB.out_slots([3 * i for i in range(16)], mis=DB.out_mis)
    assert [int(b - a) - 3 * i - 64 for i, (a, b) in enumerate(zip(ooff, ooff[1:]))] == [DB.out_mis(i + 1) for i in range(15)]


def test_output_layout_is_these_numbers():
    ooff, total = DB.out_slots(CAPS)
    assert ooff.tolist() == OOFF and total == 537 + 64
    ooff, total = DB.out_slots(CAPS, mis=DB.out_mis)
    assert ooff.tolist() == [64, 135, 214, 299, 391, 498] and total == 578 + 64
    ooff, total = DB.out_slots(CAPS, guard=0, slots=[16, 16, 16, 16, 48, 16])      # slots of another size than the capacities, no gap
    assert ooff.tolist() == [0, 16, 32, 48, 64, 112] and total == 128 + 64
    ooff, total = DB.out_slots(CAPS, guard=32, tail=0)
    assert ooff.tolist() == [32, 64, 97, 145, 193, 265] and total == 313


def test_the_mask():
    keep = DB.untouched(OOFF, WANT, 601)
    assert keep.sum() == 601 - sum(LENS[:5]) and keep[353 + 17] and not keep[353 + 16] and keep[457]
    assert DB.untouched(OOFF, WANT, 601, written=CAPS).sum() == 601 - sum(LENS[:5]) - 16
    assert DB.untouched(OOFF, WANT, 601, sized=True).all()
    assert DB.untouched(OOFF, WANT, 601, sized=[False, False, False, False, True, False]).sum() == 601 - sum(LENS[:4])


# ---- a well-behaved call -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [None, DB.out_mis])
def test_a_well_behaved_call_passes(mis):
    res, out, back, blob, ooff, total = one_run(mis=mis)
    DB.check_results(res, WANT, tag)
    for i, c in enumerate(CHUNKS[:5]):
        assert out[int(ooff[i]):int(ooff[i]) + len(c)].tobytes() == c
    assert DB.guards_intact(out, ooff, CAPS) is None
    DB.check_mask(out, DB.untouched(ooff, WANT, total), ooff, tag)
    assert (back == blob).all()
    assert (out == 0xA5).sum() == total - sum(LENS[:5])


def test_a_dictionary_lies_3_bytes_off_a_granule_and_further_rows_and_buffers_are_freed():
    eng = Engine()
    blob, off, lens = DB.pack(CHUNKS)
    ooff, total = DB.out_slots(CAPS)
    with DB.device_batch(eng, blob, off, lens, ooff, CAPS, total, dictionary=b"dict") as b:
        assert b.d_dict % 16 == 3 and bytes(eng.mem[b.d_dict:b.d_dict + 4]) == b"dict"
        second = b.buffer(100, DB.FILL)
        r5, r6 = b.rows(ooff, lens)
        r7 = b.result_row()
        assert len(eng.live) == 7 and bytes(eng.mem[second:second + 100]) == b"\xa5" * 100
        assert b.read_row(r6).tolist() == list(LENS) and b.read_row(r7).tolist() == [DB.UNWRITTEN] * 6
        assert b.read_row(b.args[6]).tolist() == [DB.UNWRITTEN] * 6
    assert not eng.live


# ---- each fault is caught and named --------------------------------------------------------------------------------------------------------------
def poke(where):
    def fault(mem, d_in, d_out):
        mem[d_out + where] = 0x00
    return fault


def mask_failure(out, ooff, total, **kw):
    with pytest.raises(AssertionError) as ex:
        DB.check_mask(out, DB.untouched(ooff, WANT, total, **kw), ooff, tag)
    return ex.value.args[0]


def test_a_byte_in_front_of_a_slot():
    """the byte at ooff[i] - 1 is the last guard byte behind slot i - 1: reported there, at offset cap + 63 (in front of slot 0: at -1)"""
    res, out, _, _, ooff, total = one_run(poke(OOFF[3] - 1))
    assert DB.guards_intact(out, ooff, CAPS) == 2
    assert mask_failure(out, ooff, total) == ("a byte outside [0, result) changed", 16 + 63, 1, ("chunk", 2))
    res, out, _, _, ooff, total = one_run(poke(OOFF[0] - 1))
    assert DB.guards_intact(out, ooff, CAPS) == 0
    assert mask_failure(out, ooff, total) == ("a byte outside [0, result) changed", -1, 1, ("chunk", 0))


def test_a_byte_behind_a_slots_capacity():
    res, out, _, _, ooff, total = one_run(poke(OOFF[2] + 16))
    assert DB.guards_intact(out, ooff, CAPS) == 2
    assert mask_failure(out, ooff, total) == ("a byte outside [0, result) changed", 16, 1, ("chunk", 2))


def test_a_byte_behind_the_result_inside_the_capacity():
    """the guards do not see it; the mask does"""
    res, out, _, _, ooff, total = one_run(poke(OOFF[4] + 17))
    DB.check_results(res, WANT, tag)
    assert DB.guards_intact(out, ooff, CAPS) is None
    assert mask_failure(out, ooff, total) == ("a byte outside [0, result) changed", 17, 1, ("chunk", 4))


def test_a_result_that_is_never_written_is_a_mismatch_where_0_was_expected():
    res, _, _, _, _, _ = one_run(skip_result=(0,))
    assert res[0] == DB.UNWRITTEN and WANT[0] == 0
    with pytest.raises(AssertionError) as ex:
        DB.check_results(res, WANT, tag)
    assert ex.value.args[0] == (1, [("chunk", 0)])


def test_an_input_byte_changed():
    def fault(mem, d_in, d_out):
        mem[d_in + 58 + 3] ^= 0x80
    res, out, back, blob, ooff, total = one_run(fault)
    DB.check_results(res, WANT, tag)
    assert np.nonzero(back != blob)[0].tolist() == [61]


def test_a_refused_chunk_that_writes_inside_its_slot():
    def fault(mem, d_in, d_out):
        mem[d_out + OOFF[5]:d_out + OOFF[5] + 3] = b"abc"
    res, out, _, _, ooff, total = one_run(fault)
    DB.check_results(res, WANT, tag)
    assert DB.guards_intact(out, ooff, CAPS) is None
    DB.check_mask(out, DB.untouched(ooff, WANT, total, written=CAPS), ooff, tag)
    DB.check_mask(out, DB.untouched(ooff, WANT, total, written=[0, 0, 0, 0, 0, 3]), ooff, tag)
    assert mask_failure(out, ooff, total) == ("a byte outside [0, result) changed", 0, 3, ("chunk", 5))
    assert mask_failure(out, ooff, total, written=[0, 0, 0, 0, 0, 2]) == ("a byte outside [0, result) changed", 2, 1, ("chunk", 5))


# ---- nothing leaks -------------------------------------------------------------------------------------------------------------------------------
def test_a_call_that_raises_leaves_no_allocation():
    eng = Engine()
    blob, off, lens = DB.pack(CHUNKS)
    ooff, total = DB.out_slots(CAPS)

    def call(*a):
        assert len(eng.live) == 3
        raise ValueError("the call failed")
    with pytest.raises(ValueError):
        DB.run(eng, call, blob, off, lens, ooff, CAPS, total)
    assert not eng.live
    with pytest.raises(ZeroDivisionError):
        with DB.device_batch(eng, blob, off, lens, ooff, CAPS, total, dictionary=b"d") as b:
            b.buffer(10); b.result_row()
            assert len(eng.live) == 6
            1 // 0
    assert not eng.live


# ---- run_child -------------------------------------------------------------------------------------------------------------------------------------
def _script(tmp_path, code):
    p = os.path.join(str(tmp_path), "child.py")
    with open(p, "w") as f:
        f.write("import sys\n" + code)
    return p


def test_run_child(tmp_path):
    r = DB.run_child(_script(tmp_path, "print('it: ok', sys.argv[1])\nsys.exit(0)\n"), "it: ok", 60, "arg")
    assert "it: ok arg" in r.stdout
    with pytest.raises(AssertionError):
        DB.run_child(_script(tmp_path, "print('it: ok')\nsys.exit(3)\n"), "it: ok", 60)
    with pytest.raises(AssertionError):
        DB.run_child(_script(tmp_path, "print('it: almost')\nsys.exit(0)\n"), "it: ok", 60)
