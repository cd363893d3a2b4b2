"""The launch rows of every plan flavour, against a snapshot taken before the
engine's stage tables were unified (host-only, no GPU).

The stage matrix of ``tools/plan_snapshot.py`` serialises, for every plan
flavour (plain, composite, the wire pairs with and without grouped converting
kernels, scaled, keep, split / join with and without grouped launches) on
aligned and on offset pointers, the rows of ``pa_plan_stage_launches`` and
``pa_plan_stage_launches_soa``, the kernel-kind query of every entry behind
them and the error texts, and reduces each case to a SHA-256 plus a short
locator per query.  The fixture was written by that tool from the commit it
names and is never regenerated from later code."""

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
with open(snap.STAGE_FIXTURE) as _fh:
    FIXTURE = json.load(_fh)


def test_fixture_covers_the_matrix():
    assert FIXTURE["queries"] == list(snap.STAGE_QUERIES)
    assert sorted(FIXTURE["cases"]) == \
        sorted(snap.stage_case_id(c) for c in snap.stage_case_names())
    assert len(FIXTURE["generated_from_commit"]) == 40  # a clean commit


@pytest.mark.parametrize("case", snap.stage_case_names(),
                         ids=snap.stage_case_id)
def test_stages_match_snapshot(case):
    name = snap.stage_case_id(case)
    want = FIXTURE["cases"][name]
    got = list(snap.record_stage_case(*case).digest())
    if got != want:
        query = snap.first_difference(want, got, snap.STAGE_QUERIES)
        pytest.fail(
            f"case {name}: first differing query: "
            f"{query or '(digest differs, every locator matches)'}; "
            f"`python tools/plan_snapshot.py --stage --dump {name}` on both "
            f"commits shows the answers")
