"""SimpleICP.run and run_batch ask of the backend, log and return or raise what they did before their options and their
preparation were unified: every case of tests/call_sequences.py against tests/golden/call_sequences.json, which
oracle/record_call_sequences.py recorded on the commit before that change."""
import json
from pathlib import Path

import pytest

import call_sequences

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "call_sequences.json").read_text())
GOLDEN_SHARDED = json.loads((Path(__file__).resolve().parent / "golden" / "call_sequences_sharded.json").read_text())
CASES = call_sequences.cases()


def _plain(rec):
    """A fresh record as JSON hands it back (tuples are lists there)."""
    return json.loads(json.dumps(rec))


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(CASES) and sorted(GOLDEN_SHARDED) == sorted(call_sequences.SHARDED_CASES)
    assert all(sorted(GOLDEN[name]) == (["run_batch"] if case.get("batch_only") else ["run", "run_batch"]) for name, case in CASES.items())


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_batch_with_one_host_pair(name, monkeypatch):
    got, want = _plain(call_sequences.record_batch(CASES[name], monkeypatch)), GOLDEN[name]["run_batch"]
    for key in sorted(want):                      # (part by part, so that a failure names the part)
        assert got[key] == want[key], key
    assert got == want


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if not c.get("batch_only")))
def test_run(name, monkeypatch):
    got, want = _plain(call_sequences.record_run(CASES[name], monkeypatch)), GOLDEN[name]["run"]
    for key in sorted(want):
        assert got[key] == want[key], key
    assert got == want


@pytest.mark.parametrize("name", sorted(call_sequences.SHARDED_CASES))
def test_run_as_one_rank_of_a_distributed_job(name, monkeypatch):
    got, want = _plain(call_sequences.record_sharded_run(CASES[name], monkeypatch)), GOLDEN_SHARDED[name]
    for key in sorted(want):
        assert got[key] == want[key], key
    assert got == want
