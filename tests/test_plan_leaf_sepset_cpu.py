"""The planner's LEAF SEPSET mark (csrc/pgbp_plan.cpp, FEntry::pad[3], pgbp_plan_leaf_sepset): exactly the preorder records of
the register-resident kernels that send into a leaf of the schedule tree whose own postorder message integrates nothing and
fills its sepset (ni == 0, s == mf); the expectation is worked out from the description alone (leaf_sepset_cases.py)."""
import numpy as np
import pytest

import leaf_sepset_cases as K

CASES = [("cliquetree", "random", 2, 16), ("cliquetree", "random", 3, 16), ("cliquetree", "random", 40, 16),
         ("cliquetree", "random", 45, 4), ("cliquetree", "random", 50, 8), ("cliquetree", "poly6", 70, 16),
         ("cliquetree", "caterpillar", 30, 16), ("bethe", "random", 50, 16), ("edge", "", 2, 16), ("edge", "", 2, 7)]


@pytest.mark.parametrize("graph,kind,ntips,p", CASES)
def test_marked_records_are_the_leaf_receivers(graph, kind, ntips, p):
    prob = K.problem(graph, kind, ntips, p)
    marks, _ = K.plan_marks(prob)
    want = K.leaf_messages(prob)
    post_msgs, post_marked = marks[0]
    pre_msgs, pre_marked = marks[1]
    assert not post_marked, "a postorder record is never marked"
    assert pre_marked == want & pre_msgs
    if kind == "poly6":
        # tasks of five and six messages are generic-class, and a level that mixes the classes below the split threshold
        # goes to the wave-per-task kernel whole: whatever is left on the register-resident kernel obeys the rule above
        assert want
    elif ntips > 2 or graph == "edge":
        # not vacuous: these graphs run on the register-resident kernels and have such leaves
        assert want and want <= pre_msgs and len(pre_marked) == len(want)
    else:
        assert not pre_msgs   # (the 2-tip clique tree: every belief is a constant, nothing is fast-class)
    if graph == "bethe":
        assert any(p == int(prob.dims[c]) for c in prob.schedule[0][1]), "variable clusters and leaf factors of p variables"


def test_a_leaf_larger_than_its_sepset_is_not_marked():
    prob = K.tall_leaves_problem(12, 16)
    pa, ch = prob.schedule[0]
    leaves = [int(c) for c in ch if int(c) not in set(int(x) for x in pa)]
    assert leaves and all(int(prob.dims[c]) == 32 for c in leaves)
    marks, _ = K.plan_marks(prob)
    assert marks[1][0], "the tree runs on the register-resident kernels"
    assert not marks[0][1] and not marks[1][1]


def test_generic_class_records_are_not_marked():
    prob = K.generic_star()
    assert len(K.leaf_messages(prob)) == 2, "both leaves send their whole belief"
    marks, _ = K.plan_marks(prob)
    for d in (0, 1):
        assert not marks[d][0] and not marks[d][1], "no register-resident record at all, and no mark"


def test_the_tuning_key_is_read(monkeypatch):
    """leaf_sepset takes 0 or 1; the plan (the marks) does not depend on it -- the engine decides whether to honour them"""
    prob = K.problem("cliquetree", "random", 9, 16)
    base, _ = K.plan_marks(prob)
    for v in ("leaf_sepset=0", "leaf_sepset=1"):
        monkeypatch.setenv("PGBP_TUNING", v)
        got, _ = K.plan_marks(prob)
        assert got == base
    monkeypatch.setenv("PGBP_TUNING", "leaf_sepset=2")
    with pytest.raises(AssertionError):
        K.plan_marks(prob)
