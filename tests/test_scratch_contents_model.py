"""The list behind the cj_debug_scratch_* exports (csrc/cj_engine.hpp: kEngineBufs) against its two sources, without
a GPU: every cj::DevBuf and cj::PinnedBuf member of the cj_engine struct is listed — a buffer added later cannot be forgotten by the
fills of tests/test_scratch_contents_gpu.py — and the buffers the exports mark as state carriers are the ones the audit table of
DESIGN.md gives that verdict."""
import os
import re

from conftest import ROOT
from cramjam_amd import _native as N

HPP = os.path.join(ROOT, "cramjam_amd", "csrc", "cj_engine.hpp")


def exported():
    """[(name, carries_state)] in the exports' order"""
    L = N.lib()
    return [(L.cj_debug_scratch_name(i).decode(), L.cj_debug_scratch_carries_state(i)) for i in range(L.cj_debug_scratch_count())]


def struct_members():
    """the names declared `cj::DevBuf a, b;` / `cj::PinnedBuf a;` inside `struct cj_engine { ... };`, in order"""
    text = open(HPP).read()
    body = re.search(r"^struct cj_engine \{(.*?)^\};", text, re.S | re.M).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for decl in re.finditer(r"\bcj::(?:DevBuf|PinnedBuf)\s+([^;]+);", body):
        names += [n.strip() for n in decl.group(1).split(",")]
    return names


def design_table():
    """{buffer: verdict cell} of the table in DESIGN.md 5.10b"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 5.10b"):text.index("### 5.11 ")]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"\| `([dh]_[a-z_0-9]+)`[^|]*\|", line)
        if m:
            rows[m.group(1)] = line.rstrip().rstrip("|").rsplit("|", 1)[1]
    return rows


def test_every_buffer_of_the_engine_is_listed_once():
    names = [n for n, _ in exported()]
    members = struct_members()
    assert len(members) >= 25 and all(re.fullmatch(r"[dh]_[a-z_0-9]+", n) for n in members), members
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(members), sorted(set(names) ^ set(members))
    L = N.lib()
    assert L.cj_debug_scratch_name(-1) is None and L.cj_debug_scratch_name(len(names)) is None
    assert L.cj_debug_scratch_carries_state(-1) == -1 and L.cj_debug_scratch_carries_state(len(names)) == -1


def test_state_carriers_are_the_ones_the_audit_names():
    rows = design_table()
    listed = dict(exported())
    assert set(listed) <= set(rows), sorted(set(listed) - set(rows))            # every member has a row (h_meta, a std::vector, has one too)
    assert set(rows) - set(listed) == {"h_meta"}
    for name, verdict in rows.items():
        assert ("STATE" in verdict) != ("W<R" in verdict), (name, verdict)       # one verdict per row, and none is "read before written"
    assert {n for n, v in rows.items() if "STATE" in v} == {n for n, s in listed.items() if s == 1}
    assert listed["h_count"] == 1


def test_fill_refuses_a_null_list_and_peek_an_index_outside():
    L = N.lib()
    assert L.cj_debug_scratch_fill(None, 0, None) == -101                           # CJ_E_BAD_ARG, before any engine is looked for
    assert L.cj_debug_scratch_peek(None, -1, 0, None, 0) == -101 and L.cj_debug_scratch_peek(None, L.cj_debug_scratch_count(), 0, None, 0) == -101
