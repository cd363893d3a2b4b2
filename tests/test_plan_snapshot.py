"""Everything the two planners expose, against a snapshot taken before their
block tables were unified (host-only, no GPU).

``tools/plan_snapshot.py`` serialises, for a fixed matrix of plans, every
public query of the Python and the native planner and reduces each case to a
SHA-256 plus a short locator per query.  The fixture was written by that tool
from the commit it names and is never regenerated from later code: a change
of any descriptor, offset, count, launch row, kernel kind or error text of
these plans shows up here, with the case and the first query that differs."""

from __future__ import annotations

import importlib.util
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "plan_snapshot", os.path.join(REPO, "tools", "plan_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


snap = _tool()
with open(snap.FIXTURE) as _fh:
    FIXTURE = json.load(_fh)


def test_fixture_covers_the_matrix():
    assert FIXTURE["queries"] == list(snap.QUERIES)
    assert sorted(FIXTURE["cases"]) == \
        sorted(snap.case_id(c) for c in snap.case_names())
    assert len(FIXTURE["generated_from_commit"]) == 40  # a clean commit


@pytest.mark.parametrize("case", snap.case_names(), ids=snap.case_id)
def test_plans_match_snapshot(case):
    name = snap.case_id(case)
    want = FIXTURE["cases"][name]
    got = list(snap.record_case(*case).digest())
    if got != want:
        query = snap.first_difference(want, got)
        pytest.fail(
            f"case {name}: first differing query: "
            f"{query or '(digest differs, every locator matches)'}; "
            f"`python tools/plan_snapshot.py --dump {name}` on both commits "
            f"shows the answers")
