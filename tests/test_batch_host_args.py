"""The argument handling of the CPython host layer's batch entries (_cramjam.batch_host / batch_host_into), the error text helper and
the shard loop of cramjam_amd.batch — no device: engine handle 0, and every case returns or raises before any native call."""
import pytest

from cramjam_amd import _cramjam as M
from cramjam_amd import _native as N
from cramjam_amd import batch


def _host(inputs, caps, *tail):
    return M.batch_host(0, 0, 0, 0, inputs, caps, *tail)


def _into(inputs, caps, *tail, out=None, offsets=None):
    return M.batch_host_into(0, 0, 0, 0, inputs, caps, bytearray(64) if out is None else out, offsets, *tail)


ENTRIES = [_host, _into]


def test_empty_batches_return_without_a_call():
    assert M.batch_host(0, 0, 0, 0, [], []) == ([], [])
    assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), None) == []
    assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(0)) == []
    assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), []) == []
    assert M.batch_host(0, 0, 0, 0, (), (), 0, b"") == ([], [])                     # (a Blosc batch)
    for d in (b"", b"dictionary", bytearray(b"dictionary"), memoryview(b"dictionary")):        # (LZ4 blocks against a dictionary)
        assert M.batch_host(0, 0, 0, 0, [], [], 0, None, d) == ([], [])
        assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), None, 0, None, d) == []
    assert M.batch_host(0, 0, 0, 0, [], [], 0, None, None) == ([], [])
    for one_op in (True, False, 1, 0):                                              # (the signature without `op`: DEFLATE compress)
        assert M.batch_host(0, 0, 0, 0, [], [], 0, None, None, one_op) == ([], [])
        assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), None, 0, None, None, one_op) == []
    for extra in (None, 0, 1, 262144, 2 ** 32 - 1, True):                           # (the signature with a word behind flags: ORC's block size)
        assert M.batch_host(0, 0, 0, 0, [], [], 0, None, None, False, extra) == ([], [])
        assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), None, 0, None, None, False, extra) == []


@pytest.mark.parametrize("entry", ENTRIES)
def test_lengths_that_differ(entry):
    with pytest.raises(ValueError):
        entry([b"a", b"b"], [1])
    with pytest.raises(ValueError):
        entry([], [1])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("params", [b"x", bytes(19), bytes(21)])
def test_params_of_a_wrong_length(entry, params):
    with pytest.raises(ValueError):
        entry([b"a"], [1], 0, params)
    with pytest.raises(ValueError):
        entry([], [], 0, params)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("dictionary", [5, "text", 1.5, [1, 2], memoryview(bytes(8))[::2]])
def test_a_dictionary_that_is_no_contiguous_buffer(entry, dictionary):
    with pytest.raises((TypeError, BufferError)) as ex:
        entry([b"a"], [1], 0, None, dictionary)
    assert ex.type is TypeError or isinstance(dictionary, memoryview)              # (the strided view: BufferError, as for an input)
    with pytest.raises((TypeError, BufferError)):
        entry([], [], 0, None, dictionary)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("params", [b"", bytes(20)])
def test_a_dictionary_together_with_params(entry, params):
    for inputs, caps in (([b"a"], [1]), ([], [])):
        with pytest.raises(ValueError):
            entry(inputs, caps, 0, params, b"dictionary")
        with pytest.raises(ValueError):
            entry(inputs, caps, 0, params, b"")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("params, dictionary", [(b"", None), (bytes(20), None), (None, b"dictionary"), (None, b""), (bytes(20), b"dictionary")])
def test_one_op_together_with_params_or_a_dictionary(entry, params, dictionary):
    for inputs, caps in (([b"a"], [1]), ([], [])):
        with pytest.raises(ValueError):
            entry(inputs, caps, 0, params, dictionary, True)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("params, dictionary, one_op", [(b"", None, False), (bytes(20), None, False), (None, b"dictionary", False), (None, b"", False),
                                                        (None, None, True), (bytes(20), b"dictionary", True)])
def test_extra_together_with_params_a_dictionary_or_one_op(entry, params, dictionary, one_op):
    for inputs, caps in (([b"a"], [1]), ([], [])):
        for extra in (0, 4096):
            with pytest.raises(ValueError):
                entry(inputs, caps, 0, params, dictionary, one_op, extra)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("extra, error", [(1.5, TypeError), ("4096", TypeError), (b"", TypeError), ([4096], TypeError), (-1, OverflowError), (2 ** 32, OverflowError)])
def test_an_extra_that_is_no_32_bit_integer(entry, extra, error):
    for inputs, caps in (([b"a"], [1]), ([], [])):
        with pytest.raises(error):
            entry(inputs, caps, 0, None, None, False, extra)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("inputs, caps", [([b"a", 5], [1, 1]), ([b"a", None], [1, 1]), ([b"a", "text"], [1, 1]),
                                          ([b"a", b"b"], [1, -1]), ([b"a", b"b"], [1, 1.5]), ([b"a", b"b"], [1, "1"]), ([b"a", b"b"], [1, None])])
def test_an_input_that_is_no_buffer_or_a_capacity_that_is_no_size(entry, inputs, caps):
    with pytest.raises((TypeError, ValueError, OverflowError)):
        entry(inputs, caps)


def test_into_offsets_of_the_wrong_length():
    for offs in ([0], [0, 1, 2], []):
        with pytest.raises(ValueError):
            _into([b"a", b"b"], [1, 1], offsets=offs)


def test_into_out_too_small():
    with pytest.raises(ValueError):
        _into([b"a", b"b"], [4, 5], out=bytearray(8))                               # back to back: 4 + 5 > 8
    with pytest.raises(ValueError):
        _into([b"a", b"b"], [4, 4], out=bytearray(8), offsets=[0, 5])
    with pytest.raises(ValueError):
        _into([b"a"], [0], out=bytearray(8), offsets=[9])
    with pytest.raises(ValueError):
        _into([b"a"], [2 ** 64 - 1], out=bytearray(8), offsets=[2])                # (offset + capacity wraps)


def test_into_read_only_out():
    for out in (bytes(8), memoryview(bytearray(8)).toreadonly()):
        with pytest.raises(ValueError):
            _into([b"a"], [1], out=out)


def _failing(first, d=None, extra=None):
    """calls that fail on the entry BEHIND `first`, whose buffer has been borrowed by then (d: while a dictionary is borrowed too; extra:
    in the signature with a word behind flags)"""
    tail = (0, None, None, False, extra) if extra is not None else () if d is None else (0, None, d)
    yield lambda: _host([first, 5], [1, 1], *tail)
    yield lambda: _host([first, b"b"], [1, -1], *tail)
    yield lambda: _into([first, 5], [1, 1], *tail)
    yield lambda: _into([first, b"b"], [1, -1], *tail)
    yield lambda: _into([first, b"b"], [8, 8], *tail, out=bytearray(12))
    yield lambda: _into([first, b"b"], [1, 1], *tail, offsets=[0, "x"])
    yield lambda: _into([first, b"b"], [1, 1], *tail, offsets=[0])
    yield lambda: _host([first, b"b"], [1], *tail)
    if extra is not None:
        yield lambda: _into([first], [1], *tail, out=bytes(8))           # (a read-only out)
    elif d is None:
        yield lambda: _host([first], [1], 0, b"xyz")
    else:
        yield lambda: _host([first], [1], 0, b"", d)                # (params and a dictionary)
        yield lambda: _into([first], [1], 0, bytes(20), d)
        yield lambda: _into([first], [1], 0, None, d, out=bytes(8))       # (a read-only out)


def test_a_failure_releases_the_inputs_it_borrowed():
    for k in range(9):
        first = bytearray(b"0123456789")
        call = list(_failing(first))[k]
        with pytest.raises((TypeError, ValueError, OverflowError)):
            call()
        first.extend(b"more")                # BufferError while a buffer export of the call is still alive
        del first[:]


def test_a_failure_with_extra_releases_the_inputs_it_borrowed():
    for k in range(9):
        first = bytearray(b"0123456789")
        call = list(_failing(first, extra=4096))[k]
        with pytest.raises((TypeError, ValueError, OverflowError)):
            call()
        first.extend(b"more")
        del first[:]


def test_a_failure_releases_the_dictionary_it_borrowed():
    for k in range(11):
        first, d = bytearray(b"0123456789"), bytearray(b"the dictionary")
        call = list(_failing(first, d))[k]
        with pytest.raises((TypeError, ValueError, OverflowError)):
            call()
        for b in (first, d):
            b.extend(b"more")
            del b[:]


def test_a_call_that_returns_releases_the_dictionary():
    d = bytearray(b"the dictionary")
    assert M.batch_host(0, 0, 0, 0, [], [], 0, None, d) == ([], [])
    assert M.batch_host_into(0, 0, 0, 0, [], [], bytearray(4), None, 0, None, d) == []
    d.extend(b"more")
    del d[:]


def test_the_hip_error_text_is_always_appended():
    """_cramjam formats "cramjam_hip error %d: %s" and leaves the HIP text to the caller, which appends it whatever the message ends
    with: cj_strerror(CJ_E_NO_DEVICE) — the code of every failed HIP call — ends with a parenthesis itself"""
    hip = N.lib().cj_last_hip_error().decode()
    no_device = "cramjam_hip error %d: %s" % (N.E_NO_DEVICE, N.strerror(N.E_NO_DEVICE))
    assert no_device.endswith(")")
    for msg in (no_device, "cramjam_hip error -101: cramjam_hip: bad argument", ""):
        assert N._with_hip_error(msg) == "%s (%s)" % (msg, hip)


@pytest.mark.parametrize("n", [0, 1, 2, 5])
@pytest.mark.parametrize("g", [1, 2, 3])
def test_shard_visits_every_index_once_and_keeps_the_callers_order(n, g):
    devices = ["dev%d" % k for k in range(g)]
    seen = []

    def work(dev, idx):
        idx = list(idx)
        seen.append((dev, idx))
        return [i * 10 for i in idx], [(dev, i) for i in idx]

    a, b = batch._shard(devices, n, work)
    assert list(a) == [i * 10 for i in range(n)]
    assert list(b) == [(devices[i % g], i) for i in range(n)]                       # index i went to device i mod G
    assert sorted(i for _, idx in seen for i in idx) == list(range(n))
    assert sorted(dev for dev, _ in seen) == devices                                # one piece of work per device
    assert batch._shard(None, n, lambda dev, idx: ([dev] * len(idx),)) == ([0] * n,)        # (no devices given: device 0)


# ---- the argument lists of the Kinds (_native.Kind.device_args / sizes_args): h, i, o, result, stream are stand-ins ---------------------------
I, O = ("in", "ioff", "ilen"), ("out", "ooff", "ocap")


def test_orc_puts_the_extra_word_directly_behind_flags():
    assert N.ORC.extra and N._HOST_KINDS["cj_orc_batch_host"] is N.ORC
    assert N.ORC.device_args("h", 4, 1, 0, 7, I, O, "res", None, "st", 65536) == ("h", 4, 1, 0, 65536, 7) + I + O + ("res", "st")
    assert N.ORC.sizes_args("h", 4, 0, 7, I + ("res",), ("st",), 0, 65536) == ("h", 4, 0, 65536, 7) + I + ("res", "st")
    assert N.ORC.sizes_args("h", 4, 0, 7, ("ptrs", "lens", "res"), (), extra=4096) == ("h", 4, 0, 4096, 7, "ptrs", "lens", "res")
    L = N.SYMBOLS
    assert len(L["cj_orc_batch_device"][1]) == 14 and len(L["cj_orc_sizes_device"][1]) == 10 and len(L["cj_orc_sizes_host"][1]) == 8


def test_every_other_kinds_argument_lists_are_unchanged():
    for kind in (N.BLOCKS, N.FRAMES, N.DEFLATE, N.ZSTD, N.BGZF):
        assert not kind.extra
        for extra in (None, 65536):                                                 # (a word the kind does not take is not passed on)
            assert kind.device_args("h", 2, 1, 9, 7, I, O, "res", None, "st", extra) == ("h", 2, 1, 9, 7) + I + O + ("res", "st")
            assert kind.sizes_args("h", 2, 9, 7, I + ("res",), ("st",), 0, extra) == ("h", 2, 9, 7) + I + ("res", "st")
        assert kind.sizes_args("h", 2, 9, 7, ("ptrs", "lens", "res")) == ("h", 2, 9, 7, "ptrs", "lens", "res")
    for kind in (N.DEFLATE_COMPRESS, N.ZSTD_COMPRESS):
        assert kind.device_args("h", 2, 1, 9, 7, I, O, "res", None, "st") == ("h", 2, 9, 7) + I + O + ("res", "st")
    assert N.DICT.device_args("h", 0, 1, 9, 7, I, O, "res", ("dict", 5), "st") == ("h", 0, 1, 9, 7) + I + O + ("res", "dict", 5, "st")
    assert N.DICT.sizes_args("h", 0, 9, 7, I + ("res",), ("st",), 5) == ("h", 0, 9, 7) + I + ("res", 5, "st")
    assert N.DICT.sizes_args("h", 0, 9, 7, ("ptrs", "lens", "res"), (), 5) == ("h", 0, 9, 7, "ptrs", "lens", "res", 5)
    assert N.BLOSC.device_args("h", 0, 1, 9, 7, I, O, "res", None, "st") == ("h", 1) + I + O + ("res", 7, None, 9, "st")
    assert N.BLOSC.sizes_args("h", 0, 9, 7, I + ("res",), ("st",)) == ("h", 9, 7) + I + ("res", "st")
    assert [k for k in N._HOST_KINDS.values() if k.extra] == [N.ORC]


def test_the_engine_refuses_an_extra_word_the_kind_does_not_take_and_a_missing_one():
    e = N.Engine.__new__(N.Engine)
    e.h = None                                                                      # (no device: the checks come before the handle is read)
    with pytest.raises(ValueError):
        N.Engine.batch_host(e, 0, 0, 0, [], [], N.BGZF, extra=4096)
    with pytest.raises(ValueError):
        N.Engine.batch_host(e, N.ORC_ZLIB, 0, 0, [], [], N.ORC)
    with pytest.raises(ValueError):
        N.Engine.batch_host_into(e, N.ORC_ZLIB, 0, 0, [], [], bytearray(4), None, N.ORC)
