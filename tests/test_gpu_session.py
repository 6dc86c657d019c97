"""One long-lived context through seeded sessions of mixed operations (tests/session_model.py): every state change the API offers, in an order
nobody scripted, and behind each of them observations that are checked on every bit against the host twins and the oracle over a model of
plain data.  What this looks for gives a wrong answer and no fault: a tile cover or an exposure mask that outlives its tree version, a BVH2
read back stale, a small batch that reads what a larger one of another family left in a shared buffer, an arena laid out for another count.

Each case is one session in a process of its own, because the torch routes need torch imported before the package (as the *_torch_cases.py
modules do it); the session creates ONE context and closes it at its end.  On a mismatch the message carries the seed, the step and the
operation log up to that step; session_model.run(seed, stop_after=step) replays the prefix."""
import os
import subprocess
import sys

import pytest

import session_model as sm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_session(seed):
    """LENGTH operations on one context; every observation is checked where it happens, and at the end the session's own coverage
    (session_model.check_coverage: the conditions tests/test_session_model.py checks on the records, and the three that need the device --
    a current exposure mask before an update and after one, a large launch while the mask was stale).  The mismatch message ends, as it
    begins, with the line that says what differed, so the tail kept here always holds it."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "session_model.py"), "gpu", str(seed)], capture_output=True, text=True, timeout=600, cwd=HERE)
    assert r.returncode == 0 and ("ok session %d: %d operations" % (seed, sm.LENGTH)) in r.stdout, r.stdout[-3000:] + r.stderr[-20000:]
    print(r.stdout.strip().splitlines()[-1])
