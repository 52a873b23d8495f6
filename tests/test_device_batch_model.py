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


# ---- the far placement -----------------------------------------------------------------------------------------------------------------------------
BITS, MARGIN = 20, 256                              # the stand-in's line: 2^20, so its two allocations are 1.5 MiB + 16 KiB each
H, L = 1 << (BITS - 1), 1 << BITS
FAR_LENS = (40, 300, 33, 90, 17, 1, 64, 129, 250, 31, 2, 77, 100, 210, 5, 0, 55, 16, 48, 9)
FAR = [dict(bytes=bytes((i * 37 + j * (i + 3)) % 250 + 1 for j in range(n)), cap=n + (i % 3) * 7, result=n) for i, n in enumerate(FAR_LENS)]
for _c in FAR:
    _c["out"] = _c["bytes"]
FAR[7] = dict(FAR[7], cap=100, result=-3, out=b"")  # (place D) does not fit: refused
far_tag = lambda i, got: ("case", i, "got", got)
sext = lambda v: v % L - L if v % L >= H else v % L


def far_kernel(eng, in_at=lambda o, k: o + k, out_at=lambda o, k: o + k):
    """copies chunk by chunk, byte k of a chunk at in_at(in_off, k) and out_at(out_off, k): the right kernel, or one wrong address"""
    def call(idx, d_in, in_off, in_len, d_out, out_off, out_cap, result):
        n = len(idx)
        row = lambda p: [int(v) for v in eng.d2h(p, 8 * n, "int64")]
        for i, (o, ln, oo, cap) in enumerate(zip(row(in_off), row(in_len), row(out_off), row(out_cap))):
            for k in range(ln if ln <= cap else 0):
                eng.mem[d_out + out_at(oo, k)] = eng.mem[d_in + in_at(o, k)]
            eng.h2d(result + 8 * i, np.int64(ln if ln <= cap else -3))
    return call


def far_run(key="far", **addr):
    eng = Engine()
    with DB.far_buffers(eng, BITS) as far:
        assert far.size == H + L + (1 << 14) and len(eng.live) == 2
        DB.run_far(eng, far, key, FAR, far_kernel(eng, **addr), far_tag, margin=MARGIN)
        assert len(eng.live) == 2
    assert not eng.live


def test_the_far_layout():
    assert DB.far_size(32) == (2 << 30) + (4 << 30) + (64 << 20) and DB.FAR_CALLS == (("A", "B", "D"), ("C",))
    seen = set()
    for places in DB.FAR_CALLS:
        F = DB.far_layout("far", FAR, BITS, places, MARGIN)
        assert [i % 4 for i in F.idx] == [DB.PLACES.index(p) for _ in range(len(F.idx) // len(places)) for p in places]
        seen |= set(F.idx)
        place = lambda p: [k for k, i in enumerate(F.idx) if DB.PLACES[i % 4] == p]
        for p, line in (("A", H), ("B", L)):
            if p in places:
                s_in, s_out = F.straddlers[p]
                assert len(s_in) == 1 and len(s_out) == 1, "one chunk of the place has its first byte below the line and its last byte above it"
                k = s_in[0]
                assert int(F.in_off[k]) < line <= int(F.in_off[k]) + int(F.in_len[k]) - 1 and F.in_len[k] == max(F.in_len[place(p)])
                k = s_out[0]
                assert int(F.out_off[k]) < line <= int(F.out_off[k]) + int(F.want[k]) - 1 and F.want[k] > 0
                assert min(F.in_off[place(p)]) < line < max(F.in_off[place(p)]) and min(F.out_off[place(p)]) < line < max(F.out_off[place(p)])
        if "C" in places:
            assert int(F.in_off[place("C")[0]]) == L and int(F.out_off[place("C")[0]]) == L
        if "D" in places:
            assert int(F.in_off[place("D")[0]]) == L + (1 << (BITS - 7)) + 5 and int(F.out_off[place("D")[0]]) == L + (1 << (BITS - 7)) + 5
        if "A" in places:                           # inside a place: pack()'s residues, out_slots()'s guards
            ks = place("A")
            assert [int(F.in_off[k] - F.in_off[ks[0]]) % 16 for k in ks] == [DB.in_mis(q) for q in range(len(ks))]
            assert all(int(F.out_off[b]) - int(F.out_off[a]) - int(F.caps[a]) == DB.G for a, b in zip(ks, ks[1:]))
        # every decoy differs from the chunk it shadows, under each truncation that moves the chunk
        for k, (j, decoy) in F.decoys.items():
            real, o = FAR[F.idx[k]]["bytes"], int(F.in_off[k])
            assert j != F.idx[k] and len(decoy) == len(real) and decoy != real
            moved = [kind for kind in ("zero", "sign") if any(a != (z if kind == "zero" else s) for a, _, z, s in DB.far_pieces(o, o + len(real), BITS))]
            assert moved and all(DB._view(real, decoy, o, BITS, kind) != real for kind in moved)
        far_in_place = [k for k, i in enumerate(F.idx) if F.in_len[k] and int(F.in_off[k]) >= H]
        assert set(far_in_place) <= set(F.decoys), "every non-empty chunk on or above 2^(bits-1) has a decoy"
        # every wrong address inside the allocation: offsets -2^(bits-1) .. 2^bits + 2^(bits-6)
        end = DB.far_size(BITS) - H
        for k in range(len(F.idx)):
            for lo, n in ((int(F.in_off[k]), int(F.in_len[k])), (int(F.out_off[k]), int(F.caps[k]))):
                for at in range(lo, lo + n):
                    assert 0 <= at < end and -H <= at % L < end and -H <= sext(at) < end
        assert all(-H <= lo < hi <= end for lo, hi, _, _ in F.in_shadows + F.out_shadows)
        kinds = {kind for _, _, _, kind in F.out_shadows}
        assert kinds == {"sign", "zero/sign"}      # (the call of place C: the guard in front of its first slot lies below the line)
    assert seen == set(range(len(FAR)))


def test_far_pieces_are_cut_at_both_lines():
    assert list(DB.far_pieces(H - 2, H + 3, BITS)) == [(H - 2, H, H - 2, H - 2), (H, H + 3, H, -H)]
    assert list(DB.far_pieces(L - 1, L + 1, BITS)) == [(L - 1, L, L - 1, -1), (L, L + 1, 0, 0)]
    assert list(DB.far_pieces(L + 9, L + 9, BITS)) == []
    assert list(DB._shadows(L - 1, L + 1, BITS)) == [(-1, 0, L - 1, "sign"), (0, 1, L, "zero/sign")]
    assert list(DB._shadows(7, H, BITS)) == []


def test_the_right_kernel_passes_at_the_far_places():
    far_run()


def far_failure(**addr):
    with pytest.raises(AssertionError) as ex:
        far_run(**addr)
    return str(ex.value.args[0])


def _case_of(msg):
    return int(msg.split("('case', ")[1].split(",")[0])


def test_in_off_cut_to_the_line_and_zero_extended():
    msg = far_failure(in_at=lambda o, k: o % L + k)
    assert msg.startswith("chunk ('case', ") and msg.endswith("read at its offset truncated to 20 bits (zero)")
    assert _case_of(msg) % 4 in (1, 3), "a chunk of place B above the line, or of place D"


def test_in_off_cut_to_the_line_and_sign_extended():
    msg = far_failure(in_at=lambda o, k: sext(o) + k)
    assert msg.endswith("read at its offset truncated to 20 bits (sign)") and _case_of(msg) == 1, "the first chunk of place B lies in [2^19, 2^20): sign-extended, just below the base"


def test_out_off_cut_to_the_line_and_zero_extended():
    msg = far_failure(out_at=lambda o, k: o % L + k)
    assert msg.startswith("chunk ('case', ") and msg.endswith("written at its offset truncated to 20 bits (zero)")
    assert _case_of(msg) % 4 in (1, 3)


def test_out_off_cut_to_the_line_and_sign_extended():
    msg = far_failure(out_at=lambda o, k: sext(o) + k)
    assert msg.endswith("written at its offset truncated to 20 bits (sign)") and _case_of(msg) == 1


wrap = lambda o, k: o - o % L + (o + k) % L        # right for a chunk's first byte, no carry out of the low 20 bits behind it


@pytest.mark.parametrize("side", ("in_at", "out_at"))
def test_an_offset_added_in_the_lines_bits_behind_the_first_byte(side):
    """only the chunk that straddles 2^20 in place B sees it"""
    F = DB.far_layout("far", FAR, BITS, DB.FAR_CALLS[0], MARGIN)
    k = F.straddlers["B"][side == "out_at"][0]
    msg = far_failure(**{side: wrap})
    assert msg.endswith("%s at its offset truncated to 20 bits (zero)" % ("read" if side == "in_at" else "written")) and _case_of(msg) == F.idx[k]


def test_a_card_too_small_for_the_far_allocations_skips_and_leaks_nothing():
    from cramjam_amd import _native as N

    class Small(Engine):
        def alloc(self, nbytes):
            if self.live:
                raise N.EngineError("out of memory")
            return Engine.alloc(self, nbytes)
    eng = Small()
    with pytest.raises(pytest.skip.Exception) as ex:
        with DB.far_buffers(eng, BITS):
            raise RuntimeError("not reached")
    assert "%d bytes" % DB.far_size(BITS) in str(ex.value) and not eng.live


def test_a_far_call_that_raises_leaves_only_the_two_allocations():
    eng = Engine()
    def call(*a):
        raise ValueError("the call failed")
    with DB.far_buffers(eng, BITS) as far:
        with pytest.raises(ValueError):
            DB.run_far(eng, far, "far", FAR, call, far_tag, margin=MARGIN)
        assert len(eng.live) == 2
    assert not eng.live


def test_a_case_without_expected_bytes_is_held_to_its_own_verify():
    """result None: any length from at_least to the capacity, and the bytes go to verify()"""
    seen = []
    cases = [dict(c) for c in FAR]
    cases[5] = dict(cases[5], result=None, at_least=1, out=None, verify=seen.append)
    eng = Engine()
    with DB.far_buffers(eng, BITS) as far:
        DB.run_far(eng, far, "far-verify", cases, far_kernel(eng), far_tag, margin=MARGIN)
        assert seen == [FAR[5]["bytes"]]
        cases[5]["at_least"] = len(FAR[5]["bytes"]) + 1
        DB._far.clear()
        with pytest.raises(AssertionError) as ex:
            DB.run_far(eng, far, "far-verify", cases, far_kernel(eng), far_tag, margin=MARGIN)
        assert ex.value.args[0][0] == "result" and ex.value.args[0][1][:2] == ("case", 5)
    DB._far.clear()
