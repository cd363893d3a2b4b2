"""Grouped split / join launches (PA_PLAN_GROUP_SOA), host side (no GPU): the
rows pa_plan_stage_launches_soa reports.

Expected rows never come from the flagged plan: the descriptors are the
Python plan's, the kernel of each comes from pa_copy_kernel_kind_soa with the
pointers the stage uses, the workgroups from the UNFLAGGED plan's rows (one
per non-empty descriptor, which is what its stage calls launch today), and
the grouping rule is restated here: SOA_LINEAR entries of one V share a row,
all SOA_TILE entries share a row, in first-appearance order, SOA_GENERIC
entries stay alone, and a keep plan's local stage ends with ONE FILL row."""

from __future__ import annotations

import math

import pytest

from keep_util import CFG_22, CFG_EMPTY, CFG_SLAB, cfg_id, keep_sets
from soa_group_util import _descs, _tup, expected_rows
from pencilarrays_amd import Pencil, Topology, native
from pencilarrays_amd.plan import build_plan, stage_descs

ID3 = (0, 1, 2)
SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN
PACK, LOCAL, UNPACK = (native.STAGE_PACK, native.STAGE_LOCAL,
                       native.STAGE_UNPACK)
LIN, TILE, GEN, FILL = (native.KERNEL_SOA_LINEAR, native.KERNEL_SOA_TILE,
                        native.KERNEL_SOA_GENERIC, native.KERNEL_FILL)
STAGES = [(SPLIT, PACK), (SPLIT, LOCAL), (JOIN, LOCAL), (JOIN, UNPACK)]
A = 256      # the address the engine assumes for a pointer it is not given
SLAB64 = ((64, 64, 64), (8,), (1,), ID3, (0,), ID3, ())
SLAB64P = ((64, 64, 64), (8,), (1,), ID3, (0,), (1, 0, 2), ())
TWO_V = ((10, 12, 5), (3,), (1,), ID3, (0,), ID3, ())


def _pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po), topo.nranks, extra)


def _plans(cfg, r, ssz, keep=None, fill=native.FILL_ZERO):
    Pi, Po, _, extra = _pencils(cfg)
    mk = lambda g: native.NativePlan(Pi, Po, r, ssz, extra, keep=keep,
                                     fill=fill, group_soa=g)
    pl = build_plan(Pi, Po, r, extra, keep=keep,
                    fill="zero" if fill else None)
    return mk(False), mk(True), pl


def _as_tuples(rows):
    return [(r.kind, r.grouped, r.entries, r.workgroups) for r in rows]


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("ssz", [4, 8, 16])
@pytest.mark.parametrize("cfg", [CFG_22, CFG_SLAB, CFG_EMPTY], ids=cfg_id)
def test_rows_follow_the_grouping_rule_on_every_rank(cfg, ssz, n):
    nr = math.prod(cfg[1])
    seen = set()
    for r in range(nr):
        flat, grp, pl = _plans(cfg, r, ssz)
        assert not flat.group_soa() and grp.group_soa()
        for d, stage in STAGES:
            # a vector-valued array one scalar past a 256-byte boundary
            for aos in (A, A + ssz):
                want, _ = expected_rows(flat, pl, n, d, stage, ssz, aos)
                got = grp.stage_launches_soa(n, d, stage, aos, [A] * n)
                assert _as_tuples(got) == want, (r, d, stage, aos)
                seen.update(w[0] for w in want)
                # only a descriptor with no contiguous axis stays ungrouped
                assert all(w[1] == (w[0] != GEN) for w in want)
    assert seen   # something was launched somewhere


def test_slab_rank0_is_one_grouped_row_of_seven():
    n, ssz = 3, 8
    flat, grp, pl = _plans(SLAB64, 0, ssz)
    rows = grp.stage_launches_soa(n, SPLIT, PACK)
    un = flat.stage_launches_soa(n, SPLIT, PACK)
    assert len(un) == 7 and all(u == (LIN, False, 1, u.workgroups)
                                for u in un)
    assert _as_tuples(rows) == [(LIN, True, 7,
                                 sum(u.workgroups for u in un))]
    flat, grp, pl = _plans(SLAB64P, 0, ssz)
    rows = grp.stage_launches_soa(n, JOIN, UNPACK)
    un = flat.stage_launches_soa(n, JOIN, UNPACK)
    assert len(un) == 7 and all(u.kind == TILE and not u.grouped for u in un)
    assert _as_tuples(rows) == [(TILE, True, 7,
                                 sum(u.workgroups for u in un))]
    # the local stage: one entry, still a grouped row
    assert _as_tuples(grp.stage_launches_soa(n, JOIN, LOCAL)) == \
        [(TILE, True, 1, flat.stage_launches_soa(n, JOIN, LOCAL)[0].workgroups)]


def test_an_empty_rank_launches_nothing():
    # 3 planes over 4 ranks: the ranks of the first row own nothing on the
    # input pencil, so they pack nothing and have no local block
    Pi, _, nr, _ = _pencils(CFG_EMPTY)
    empty = [r for r in range(nr) if Pi.length_local(r) == 0]
    assert empty
    for r in empty:
        flat, grp, pl = _plans(CFG_EMPTY, r, 8)
        for p in (flat, grp):
            assert p.stage_launches_soa(3, SPLIT, PACK) == []
            assert p.stage_launches_soa(3, SPLIT, LOCAL) == []
            assert p.stage_launches_soa(3, JOIN, LOCAL) == []


def test_a_misaligned_array_moves_to_a_lower_v_row():
    n, ssz = 3, 4
    flat, grp, pl = _plans(SLAB64, 0, ssz)
    full = grp.stage_launches_soa(n, SPLIT, PACK, 4096)
    half = grp.stage_launches_soa(n, SPLIT, PACK, 4096 + 8)
    one = grp.stage_launches_soa(n, SPLIT, PACK, 4096 + 4)
    for rows in (full, half, one):
        assert [(r.kind, r.grouped, r.entries) for r in rows] == \
            [(LIN, True, 7)]
    # a lane moves V elements: a quarter of the lanes at V = 4
    assert one[0].workgroups == 2 * half[0].workgroups == \
        4 * full[0].workgroups
    # per descriptor, the selection says the same
    desc, fp = _descs(pl, n, SPLIT, PACK, ssz, 4096, None)[0]
    for aos, v in ((4096, 4), (4096 + 8, 2), (4096 + 4, 1)):
        assert native.copy_kernel_kind_soa(_tup(desc), ssz, n, SPLIT, aos,
                                           fp).vec == v


def test_two_linear_rows_of_different_v_in_one_stage():
    """x = 10 over 3 ranks is 3 + 3 + 4: the block of 4 moves two scalars an
    access, a block of 3 one, so rank 0's pack has a row of each."""
    n, ssz = 3, 4
    cfg = TWO_V
    flat, grp, pl = _plans(cfg, 0, ssz)
    want, _ = expected_rows(flat, pl, n, SPLIT, PACK, ssz)
    got = grp.stage_launches_soa(n, SPLIT, PACK)
    assert _as_tuples(got) == want
    vs = {native.copy_kernel_kind_soa(_tup(d), ssz, n, SPLIT, A, fp).vec
          for d, fp in _descs(pl, n, SPLIT, PACK, ssz, A, None)}
    assert len(vs) >= 2 and len(got) == len(vs) and \
        all(r.kind == LIN and r.grouped for r in got)


def test_a_generic_row_beside_a_grouped_row():
    """x = 4 over 3 ranks is 1 + 1 + 2: the block one plane thick has no
    contiguous axis on the array side."""
    cfg = ((4, 12, 5), (3,), (1,), ID3, (0,), ID3, ())
    flat, grp, pl = _plans(cfg, 0, 8)
    want, _ = expected_rows(flat, pl, 2, SPLIT, PACK, 8)
    got = grp.stage_launches_soa(2, SPLIT, PACK)
    assert _as_tuples(got) == want
    assert [(g.kind, g.grouped, g.entries) for g in got] == \
        [(GEN, False, 1), (LIN, True, 1)]


@pytest.mark.parametrize("cfg", [SLAB64, SLAB64P], ids=["plain", "permuted"])
def test_n5_stays_one_generic_row_per_descriptor(cfg):
    n, ssz = 5, 8
    flat, grp, pl = _plans(cfg, 0, ssz)
    for d, stage in STAGES:
        un = flat.stage_launches_soa(n, d, stage)
        got = grp.stage_launches_soa(n, d, stage)
        assert got == un
        assert all(r.kind == GEN and not r.grouped and r.entries == 1
                   for r in got)
        assert len(got) == (1 if stage == LOCAL else 7)


@pytest.mark.parametrize("name", ["inside", "two_ranges", "two_dims"])
@pytest.mark.parametrize("cfg", [CFG_22, CFG_SLAB], ids=cfg_id)
def test_keep_plan_rows(cfg, name):
    n, ssz = 3, 8
    keep = keep_sets(cfg)[name]
    nr = math.prod(cfg[1])
    fills = 0
    for r in range(nr):
        for fill in (native.FILL_ZERO, native.FILL_NONE):
            flat, grp, pl = _plans(cfg, r, ssz, keep, fill)
            # the unflagged keep plan refuses the query like the calls
            with pytest.raises(RuntimeError, match="cannot run on a keep"):
                flat.stage_launches_soa(n, SPLIT, PACK)
            for d, stage in STAGES:
                got = grp.stage_launches_soa(n, d, stage)
                copies = [g for g in got if g.kind != FILL]
                # entries are sub-boxes: one per non-empty descriptor
                nsub = sum(1 for which, dd in stage_descs(
                    pl, n, 0, {PACK: 0, LOCAL: 1, UNPACK: 2}[stage])
                    if math.prod(dd.dims))
                assert sum(g.entries for g in copies) == nsub
                assert all(g.grouped == (g.kind != GEN) for g in got)
                nfill = grp.nfill() if fill == native.FILL_ZERO else 0
                assert nfill == len(pl.fills)
                if stage == LOCAL and nfill:
                    assert got[-1].kind == FILL and got[-1].grouped
                    assert got[-1].entries == \
                        (n * nfill if d == SPLIT else nfill)
                    assert [g.kind for g in got].count(FILL) == 1
                    fills += 1
                    # the n-field keep plan's fill row: same windows, same
                    # bytes, hence the same workgroups for a split
                    many = grp.stage_launches(n, LOCAL)[-1]
                    assert many.kind == FILL
                    if d == SPLIT:
                        assert got[-1] == many
                else:
                    assert all(g.kind != FILL for g in got)
    assert fills


def test_invalid_pairs_and_bad_arguments():
    flat, grp, _ = _plans(SLAB64, 0, 8)
    for p in (flat, grp):
        for d, stage, what in ((SPLIT, UNPACK, "unpack of a split"),
                               (JOIN, PACK, "pack of a join")):
            with pytest.raises(RuntimeError, match=what) as e:
                p.stage_launches_soa(3, d, stage)
            assert "pa_plan_stage_launches" in str(e.value)
        with pytest.raises(RuntimeError, match="n must be >= 2"):
            p.stage_launches_soa(1, SPLIT, PACK)
        with pytest.raises(RuntimeError, match="unknown direction 2"):
            p.stage_launches_soa(3, 2, PACK)
        with pytest.raises(RuntimeError, match="bad stage 3"):
            p.stage_launches_soa(3, SPLIT, 3)
        with pytest.raises(RuntimeError, match="not aligned to the 8-byte"):
            p.stage_launches_soa(3, SPLIT, PACK, 4096 + 4)
        with pytest.raises(RuntimeError, match="field 1 is not aligned"):
            p.stage_launches_soa(3, SPLIT, LOCAL, 4096, [4096, 4100, 4096])
    import ctypes
    lib = native.load()
    st = lib.pa_plan_stage_launches_soa(grp._plan, 3, SPLIT, PACK, None, None,
                                        0, None, None)
    assert st != 0 and b"null argument" in lib.pa_last_error()
    st = lib.pa_plan_stage_launches_soa(None, 3, SPLIT, PACK, None, None, 0,
                                        None, ctypes.byref(ctypes.c_int()))
    assert st != 0 and b"null plan" in lib.pa_last_error()
