"""Grouped converting kernels of a wire plan (PA_PLAN_GROUP_CVT), host only:
the flag changes the launch rows of a wire plan and nothing else.  Expected
rows are built from the unflagged plan's rows and the selection query
(wire_group_util.expected_rows), never from the flagged plan."""

import math

import numpy as np
import pytest

from pencilarrays_amd import (
    MultiTransposition, PencilArray, Transposition, build_plan, native,
    run_transpose_sim, transpose_into,
)
from wire_group_util import (
    GEN, LIN, STAGES, TILE, expected_rows, flagged_rows, pencils, wire_plan,
)
from wire_util import PAIRS, assert_same, seeded_values

ID3 = (0, 1, 2)
CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, (3,)),
]
SLAB = ((64, 64, 64), (8,), (1,), ID3, (0,), (1, 0, 2), ())
MIX5 = ((9, 16, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ())
CVT = {LIN, TILE, GEN}


def _ids(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}"


def _rows(l):
    return [(x.kind, x.grouped, x.entries) for x in l]


# ---- 1. flag off is today ----------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS, ids=_ids)
def test_flag_off_is_the_plan_without_the_argument(cfg):
    for r in range(math.prod(cfg[1])):
        a = wire_plan(cfg, r, "f64_f32", 1)
        b = wire_plan(cfg, r, "f64_f32", 1, group_cvt=False)
        assert not a.group_cvt() and not b.group_cvt()
        for s in STAGES:
            ra, rb = a.stage_launches(3, s), b.stage_launches(3, s)
            assert ra == rb
            assert all(l.kind in CVT and not l.grouped and l.entries == 1
                       for l in ra), ra


# ---- 2. tables do not depend on the flag ----------------------------------------

@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("cfg", CFGS, ids=_ids)
def test_tables_do_not_depend_on_the_flag(cfg, nc, aliased):
    Pi, Po = pencils(cfg)
    for r in range(math.prod(cfg[1])):
        a = wire_plan(cfg, r, "f64_f32", nc, aliased)
        b = wire_plan(cfg, r, "f64_f32", nc, aliased, group_cvt=True)
        assert a.plan_wire() == b.plan_wire() == PAIRS["f64_f32"][2]
        for which in range(5):
            for k in range(a.nproc_sub if which in (1, 2) else 1):
                assert a.copydesc(which, k) == b.copydesc(which, k)
                assert a.copydesc_many(3, 2, which, k) == \
                    b.copydesc_many(3, 2, which, k)
        assert a.buffer_sizes() == b.buffer_sizes()
        assert a.buffer_sizes_many(3) == b.buffer_sizes_many(3)
        for blk in build_plan(Pi, Po, r, cfg[6], aliased=aliased).peers:
            for n in (1, 3):
                assert a.peer_message(n, blk.peer_k) == \
                    b.peer_message(n, blk.peer_k)


# ---- 3. launch rows of the even slab ----------------------------------------------

def test_launch_rows_even_slab():
    n = 3
    Pi, Po = pencils(SLAB)
    for r in (0, 5):
        plain = wire_plan(SLAB, r, "f64_f32", 1)
        p = wire_plan(SLAB, r, "f64_f32", 1, group_cvt=True)
        got = flagged_rows(p, n)
        assert _rows(got[native.STAGE_PACK]) == [(LIN, True, 21)]
        assert _rows(got[native.STAGE_UNPACK]) == [(TILE, True, 21)]
        assert _rows(got[native.STAGE_LOCAL]) == [(TILE, True, 3)]
        for s in STAGES:
            assert got[s][0].workgroups == \
                sum(l.workgroups for l in plain.stage_launches(n, s))
        assert got == expected_rows(plain, build_plan(Pi, Po, r, ()), n,
                                    "f64_f32", 1)


def test_empty_rank_launches_nothing():
    cfg = CFGS[2]
    Pi, Po = pencils(cfg)
    r = next(r for r in range(8) if Pi.length_local(r) == 0)
    p = wire_plan(cfg, r, "f64_f32", 1, group_cvt=True)
    assert p.stage_launches(3, native.STAGE_PACK) == []
    assert p.stage_launches(3, native.STAGE_LOCAL) == []


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("pair,nc", [("f64_f32", 1), ("f64_f32", 2),
                                     ("f64_f32", 3), ("f32_bf16", 1)])
@pytest.mark.parametrize("cfg", CFGS, ids=_ids)
def test_rows_are_the_partition_of_the_unflagged_rows(cfg, pair, nc, aliased):
    Pi, Po = pencils(cfg)
    for r in range(math.prod(cfg[1])):
        plain = wire_plan(cfg, r, pair, nc, aliased)
        p = wire_plan(cfg, r, pair, nc, aliased, group_cvt=True)
        py = build_plan(Pi, Po, r, cfg[6], aliased=aliased)
        for n in (1, 3):
            assert flagged_rows(p, n) == \
                expected_rows(plain, py, n, pair, nc), (r, n)


# ---- 4. a field one scalar off ------------------------------------------------------

def test_misaligned_field_moves_to_its_own_linear_row():
    n = 3
    Pi, Po = pencils(SLAB)
    srcs = [0x10000, 0x20008, 0x30000]  # field 1: one f64 into its allocation
    plain = wire_plan(SLAB, 0, "f64_f32", 1)
    p = wire_plan(SLAB, 0, "f64_f32", 1, group_cvt=True)
    pack = p.stage_launches(n, native.STAGE_PACK, srcs, None)
    assert _rows(pack) == [(LIN, True, 14), (LIN, True, 7)]
    want = expected_rows(plain, build_plan(Pi, Po, 0, ()), n, "f64_f32", 1,
                         sp=srcs)
    assert pack == want[native.STAGE_PACK]
    # V = 2 moves twice the scalars per lane: the misaligned field's seven
    # entries need as many workgroups as the other fourteen together
    assert pack[1].workgroups == pack[0].workgroups
    # the tiles do not look at the source alignment
    assert _rows(p.stage_launches(n, native.STAGE_LOCAL, srcs, None)) == \
        [(TILE, True, 3)]


# ---- 5. ncomp = 5 -------------------------------------------------------------------

def test_five_components_keep_generic_rows():
    n = 3
    Pi, Po = pencils(SLAB)
    plain = wire_plan(SLAB, 0, "f64_f32", 5)
    p = wire_plan(SLAB, 0, "f64_f32", 5, group_cvt=True)
    got = flagged_rows(p, n)
    assert _rows(got[native.STAGE_PACK]) == [(LIN, True, 21)]
    assert _rows(got[native.STAGE_UNPACK]) == [(GEN, False, 1)] * 21
    assert _rows(got[native.STAGE_LOCAL]) == [(GEN, False, 1)] * 3
    assert got == expected_rows(plain, build_plan(Pi, Po, 0, ()), n,
                                "f64_f32", 5)
    # generic and grouped rows side by side in ONE stage: nine planes over
    # eight ranks leave one-plane windows with no contiguous axis (generic)
    # next to one block of runs (linear) in the pack stage; the one-plane
    # unpacks are runs again
    Pi, Po = pencils(MIX5)
    pa = wire_plan(MIX5, 0, "f64_f32", 5, aliased=True, group_cvt=True)
    got = flagged_rows(pa, n)
    pack = _rows(got[native.STAGE_PACK])
    assert sorted(set(pack)) == [(LIN, True, 3), (GEN, False, 1)]
    assert pack.count((LIN, True, 3)) == 1 and len(pack) == 1 + 7 * n
    assert _rows(got[native.STAGE_UNPACK]) == [(LIN, True, 7 * n)]
    assert got == expected_rows(
        wire_plan(MIX5, 0, "f64_f32", 5, aliased=True),
        build_plan(Pi, Po, 0, (), aliased=True), n, "f64_f32", 5)


# ---- 6. the flag on a plan without a wire pair --------------------------------------

@pytest.mark.parametrize("cfg", CFGS, ids=_ids)
def test_flag_without_a_wire_pair_changes_nothing(cfg):
    Pi, Po = pencils(cfg)
    for r in range(math.prod(cfg[1])):
        a = native.NativePlan(Pi, Po, r, 8, cfg[6])
        b = native.NativePlan(Pi, Po, r, 8, cfg[6], group_cvt=True)
        assert not a.group_cvt() and not b.group_cvt()
        for s in STAGES:
            assert a.stage_launches(3, s) == b.stage_launches(3, s)
    k = native.NativePlan(Pi, Po, 0, 8, cfg[6], keep=[(2, 1)] * 3,
                          group_cvt=True)
    assert not k.group_cvt()
    assert wire_plan(cfg, 0, "f64_f32", 1, group_cvt=True).group_cvt()
    assert wire_plan(cfg, 0, "f32_f16", 3, aliased=True,
                     group_cvt=True).group_cvt()


# ---- 7. Python ----------------------------------------------------------------------

def _host_arrays(cfg, seed):
    Pi, Po = pencils(cfg)
    nr = math.prod(cfg[1])
    srcs = [PencilArray(Pi, r, seeded_values(Pi.length_local(r), "f64_f32",
                                             seed + r)) for r in range(nr)]
    return srcs, [PencilArray.empty(Po, r) for r in range(nr)]


def test_wire_grouped_needs_a_wire_dtype():
    srcs, dsts = _host_arrays(
        ((12, 10, 8), (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ()), 1)
    for call in (lambda: Transposition(dsts[0], srcs[0], wire_grouped=True),
                 lambda: MultiTransposition(dsts, srcs, wire_grouped=True),
                 lambda: transpose_into(dsts[0], srcs[0], wire_grouped=True),
                 lambda: run_transpose_sim(dsts, srcs, wire_grouped=True)):
        with pytest.raises(ValueError, match="wire_grouped"):
            call()
    with pytest.raises(ValueError, match="keep"):
        Transposition(dsts[0], srcs[0], wire_dtype="float32",
                      keep=[(2, 1)] * 3, wire_grouped=True)


def test_host_mirror_ignores_wire_grouped():
    cfg = CFGS[0]
    srcs, d0 = _host_arrays(cfg, 7)
    _, d1 = _host_arrays(cfg, 7)
    st0, st1 = {}, {}
    run_transpose_sim(d0, srcs, st0, wire_dtype="float32")
    run_transpose_sim(d1, srcs, st1, wire_dtype="float32", wire_grouped=True)
    for r in range(4):
        assert_same(d1[r].data, d0[r].data, f"rank {r}")
        for name in ("send", "recv"):
            assert np.array_equal(st0[name][r].view(np.uint8),
                                  st1[name][r].view(np.uint8))
    one = ((12, 10, 8), (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    s, a = _host_arrays(one, 9)
    _, b = _host_arrays(one, 9)
    Transposition(a[0], s[0], wire_dtype=np.float32).execute()
    t = Transposition(b[0], s[0], wire_dtype=np.float32, wire_grouped=True)
    assert t.wire_grouped
    t.execute()
    assert_same(b[0].data, a[0].data)
