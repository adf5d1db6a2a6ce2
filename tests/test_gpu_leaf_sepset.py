"""The preorder message into a leaf of the schedule tree takes the old sepset from the leaf's own block (bp_fast16, bp_loop16;
PGBP_TUNING leaf_sepset=0 loads it), and the two kernels mark a site "not calibrated" themselves where every message of the
tree runs on them: tests/run_leaf_sepset_cases.py, with the default plan in this process and under no_tail (one launch per
level: the level instance sees every record) and no_chunks in a child process each, since the plan reads PGBP_TUNING when
an engine is created and the runner appends its own key to it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_default_plan():
    import run_leaf_sepset_cases as R
    assert "PGBP_TUNING" not in os.environ or "leaf_sepset" not in os.environ["PGBP_TUNING"]
    marked, in_chunks = R.run()
    assert marked > 0 and in_chunks > 0


@pytest.mark.parametrize("tuning", ["no_tail", "no_chunks", "loop=0"])
def test_other_launch_forms(tuning):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PGBP_TUNING"] = tuning
    out = subprocess.run([sys.executable, os.path.join(here, "run_leaf_sepset_cases.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, (tuning, out.stdout[-2000:], out.stderr[-3000:])
    assert "cases ok" in out.stdout
