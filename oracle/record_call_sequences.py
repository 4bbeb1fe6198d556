"""Writes tests/golden/call_sequences.json and tests/golden/call_sequences_sharded.json: what SimpleICP.run and run_batch ask of
the backend, log and return or raise for every case of tests/call_sequences.py, on the stand-in backends of the host tests.

    python oracle/record_call_sequences.py [TREE]

TREE: the checkout whose ``simpleicp_amd`` is recorded (default: this one).  The committed fixtures were recorded on the commit
BEFORE run / run_batch / run_tensors got one option set and one preparation; they are the behaviour that refactor had to keep.
Run it again only to pin a change of behaviour that is meant.
"""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TREE = Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else ROOT
sys.path[:0] = [str(TREE), str(ROOT), str(ROOT / "tests")]


def main():
    import call_sequences
    import simpleicp_amd
    assert Path(simpleicp_amd.__file__).resolve().parent.parent == TREE, simpleicp_amd.__file__
    with pytest.MonkeyPatch.context() as monkeypatch:
        records = {"call_sequences.json": call_sequences.record_all(monkeypatch)}
    records["call_sequences_sharded.json"] = call_sequences.record_all_sharded(pytest.MonkeyPatch.context)
    for name, out in records.items():
        path = ROOT / "tests" / "golden" / name
        path.write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
        print(f"{path}: {len(out)} cases, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
