"""Two caller streams and two host threads on one engine, one pairing per shared scratch of cj_engine (cj::ScratchTurn,
csrc/cj_engine.hpp; the lock graph and every entry's turns: DESIGN.md §2): tests/scratch_streams_child.py runs the pairings of
tests/scratch_streams_cases.py alone, interleaved from one thread and from two threads, with the slot budgets at three slots.  A
turn that did not wait for the previous user's event, or did not record its own, lets the second call's kernels store into slots the
first one's are reading: the later modes' bytes then differ from the alone run's.  tests/test_scratch_streams_model.py (no GPU)
holds the inputs, the expectations and the slice counts this test rests on."""
import os

import pytest

import device_batch as DB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("P1", "P1k", "P2", "P3", "P4", "P5", "P6", "P7", "P8")
# The child takes 7 s on an MI355X (2 s of it on the GPU, the rest imports and the cases' models: profiles/r22/README.md); forty times
# that, so that a busy machine does not turn into a reported hang, while a host deadlock on the nested locks still ends the child and
# not the suite
TIMEOUT = 300


def test_every_scratch_under_two_streams_and_two_threads():
    r = DB.run_child(os.path.join(HERE, "scratch_streams_child.py"), "scratch streams: ok, %d pairings" % len(NAMES), TIMEOUT)
    for name in NAMES:
        line = next(x for x in r.stdout.splitlines() if x.startswith(name + " ["))
        assert "alone, interleaved, threads ok" in line, line
        assert name not in ("P1", "P5") or "host beside device ok" in line, line
