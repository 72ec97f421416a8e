"""galileo-sdr-sim's option stage, byte for byte: exit code, stdout and stderr of every case of tests/golden/cli_transcript.json are what
the recorded binary gave (tools/cli_golden.py transcript made the file).  Every refusal, the conflicts between options and the
informational lines that pin the derived values (signal gain, --iq-shift, taps, AGC, oscillator) are among the cases; the order of the
messages is part of the text.  No device is touched: -e names a navigation file that does not exist."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cli_golden  # noqa: E402  (the runner only: the expected values come from the fixture)

with open(os.path.join(ROOT, "tests", "golden", "cli_transcript.json")) as _fh:
    FIXTURE = json.load(_fh)


def test_the_fixture_holds_the_tools_cases():
    assert [c["name"] for c in FIXTURE["cases"]] == [c["name"] for c in cli_golden.TRANSCRIPT_CASES]
    assert [c["argv"] for c in FIXTURE["cases"]] == [c["argv"] for c in cli_golden.TRANSCRIPT_CASES]
    assert FIXTURE["files"] == cli_golden.FILES
    assert len(FIXTURE["cases"]) >= 150 and {c["exit"] for c in FIXTURE["cases"]} == {1}


@pytest.mark.parametrize("case", FIXTURE["cases"], ids=[c["name"] for c in FIXTURE["cases"]])
def test_transcript(case):
    got = cli_golden.run_transcript_case(cli_golden.CLI, case, FIXTURE["files"])
    assert got["exit"] == case["exit"]
    assert got["stdout"] == case["stdout"]
    assert got["stderr"] == case["stderr"]
