"""ofdm_last_dispatch, string for string, against the commit recorded in tests/golden/dispatch_parent.json.

The file is the output of tools/dispatch_table.py on a build of that commit, on the MI355X: a fixed list of calls through every entry
point whose string comes from more than one launch site (chunk loops, the long-capture calls, the packets, the host pipe, empty calls
behind non-empty ones).  The host layer between the C ABI and the launchers may be rearranged; what a caller reads from
ofdm_last_dispatch may not move with it.  A change that is MEANT to alter a string regenerates the file and says so."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import dispatch_table  # noqa: E402

pytestmark = pytest.mark.gpu


def test_dispatch_strings_are_the_recorded_commits(ofdm):
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_parent.json")) as f:
        want = json.load(f)
    assert len(want["commit"]) == 40 and len(want["cases"]) >= 100
    got = dispatch_table.table()
    assert sorted(got) == sorted(want["cases"])
    wrong = {k: (got[k], v) for k, v in want["cases"].items() if got[k] != v}
    assert not wrong, wrong
