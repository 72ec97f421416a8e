"""galileo-sdr-sim's run loop on the MI355X, against recorded bytes: every combination of tests/golden/cli_chain_md5.json -- each
synthesis path (plain, run_gains, run_mpath, run_scint with echoes, run_array with scintillation) and each stage of the output chain
with and without the passes in front of it -- runs at -B 1 (the two output slots and the three row buffers wrap) and at -B 3 (the
run ends on a short batch); the two IQ files are equal to each other and to the recorded md5, and so are the --monitor and --agc-log
files at the same -B.  tools/cli_golden.py chain made the file from the binary whose behaviour is kept; nothing expected is computed
here."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cli_golden  # noqa: E402  (the runner only)

with open(os.path.join(ROOT, "tests", "golden", "cli_chain_md5.json")) as _fh:
    FIXTURE = json.load(_fh)


def test_the_fixture_holds_the_tools_cases():
    strip = lambda c: {k: v for k, v in c.items() if k != "expected"}
    assert [strip(c) for c in FIXTURE["cases"]] == cli_golden.CHAIN_CASES
    assert FIXTURE["scenario"] == cli_golden.CHAIN_SCEN and FIXTURE["files"] == cli_golden.CHAIN_FILES
    assert all(sorted(c["expected"]) == [str(b) for b in cli_golden.CHAIN_BATCHES] for c in FIXTURE["cases"])


@pytest.mark.parametrize("case", FIXTURE["cases"], ids=[c["name"] for c in FIXTURE["cases"]])
def test_chain(case):
    got = {str(b): cli_golden.run_chain_case(cli_golden.CLI, case, b, FIXTURE["files"]) for b in cli_golden.CHAIN_BATCHES}
    for key in got:
        print(case["name"], "-B", key, got[key])
    assert got["1"]["iq"] == got["3"]["iq"]
    assert got == case["expected"]
