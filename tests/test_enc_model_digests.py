"""The scalar encoder models reproduce the bytes they wrote when tests/golden/enc_model_digests.json was minted — from the models that
each carried their own copy of the matcher's round and of its driver, before tests/hostsim/enc2_round.h became the one statement of
both.  The reference is that recording, not the code under test.  CPU only."""
import json
import os

import pytest

import enc_model_digests as M
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN_DIR, "enc_model_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    return M.digests()


def test_every_entry_and_input_is_recorded(recorded):
    assert recorded["inputs"] == [name for name, _ in M.inputs()] and len(recorded["inputs"]) == len(M.SYNTH_LENS) + 3
    want = ["enc2_model_%s/R%d" % (c, R) for c in ("lz4", "snappy") for R in M.ROUNDS] + ["enc2_model_lz4_linked/h%d" % h for h in M.HISTORIES]
    want += ["dfe_model_compress/%s" % w for w in ("raw", "zlib", "gzip")] + ["zse_model_compress/flags0", "zse_model_compress/flags1"]
    assert sorted(recorded["digests"]) == sorted(want)
    for entry, rows in recorded["digests"].items():
        h = int(entry.split("/h")[1]) if "/h" in entry else 0
        assert sorted(rows) == sorted(name for name, data in M.inputs() if len(data) >= h), entry
        assert all(r >= 0 for r, _ in rows.values()), entry


def test_models_reproduce_every_digest(recorded, now):
    bad = [(entry, name) for entry, rows in recorded["digests"].items() for name, row in rows.items() if now[entry].get(name) != row]
    assert not bad and sorted(now) == sorted(recorded["digests"]), bad
