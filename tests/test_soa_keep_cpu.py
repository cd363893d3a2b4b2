"""Truncated split and join transposes, host side (no GPU).

The mirror (run_transpose_sim_split / _join with ``keep``) is checked against
references that never come from the code under test: the placement is the C
oracle per component on the numpy-masked (and ``scale_util.ref_scale``-scaled)
input, the staging is ``run_transpose_sim_many(keep=...)`` on the component
copies.  Whole buffers are compared as bit patterns, NaN for NaN-ness.  Then
the native plan flag PA_PLAN_GROUP_SOA, host only: what it accepts, what it
leaves refused, and that it changes nothing else about a plan."""

from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from keep_util import KEEP_NAMES, expected_keep, keep_sets
from soa_scale_util import KINDS, same, scale_bytes
from soa_util import interleave, join_case, split_case
from test_soa_cpu import CONFIGS, _ids
from pencilarrays_amd import (
    JoinTransposition,
    Pencil,
    PencilArray,
    SplitTransposition,
    Topology,
    native,
    run_transpose_sim_join,
    run_transpose_sim_many,
    run_transpose_sim_split,
    transpose_join_into,
    transpose_split_into,
)

ID3 = (0, 1, 2)
SENT = 0xAB
KIND_IDS = ["f32", "f64", "c128"]
SCALES = [0.5, -2.0, 1.0 / 3.0]


def cfg_keep_sets(cfg):
    """``keep_util.keep_sets`` for any config.  A keep set is a set of global
    indices and valid for any plan; the helper only needs a hop to place its
    cuts, so the same-decomposition config borrows the hop of CONFIGS[0]
    (same dims and topology)."""
    if tuple(cfg[2]) == tuple(cfg[4]):
        assert cfg[0] == CONFIGS[0][0] and cfg[1] == CONFIGS[0][1]
        return keep_sets(CONFIGS[0])
    return keep_sets(cfg)


def _pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po), topo.nranks, extra)


def _arr(P, r, raw, kind, extra, elem_dims=()):
    return PencilArray(P, r, raw.view(KINDS[kind][0]).copy(), extra,
                       elem_dims)


def _sentinel(P, r, nbytes, kind, extra, elem_dims=()):
    raw = np.full(nbytes, SENT, dtype=np.uint8)
    return PencilArray(P, r, raw.view(KINDS[kind][0]), extra, elem_dims)


def _many_staging(cfg, kind, srcs_c, exp_c, keep, fill):
    """Staging of the n-field KEEP plan on scalar sources ``srcs_c[c][r]``
    (bytes), after checking its destinations against ``exp_c``."""
    Pi, Po, nr, extra = _pencils(cfg)
    n = len(srcs_c)
    srcs = [[_arr(Pi, r, srcs_c[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [[_sentinel(Po, r, len(exp_c[c][r]), kind, extra)
             for c in range(n)] for r in range(nr)]
    staging = {}
    run_transpose_sim_many(dsts, srcs, staging_out=staging, keep=keep,
                           fill=fill)
    for r in range(nr):
        for c in range(n):
            same(dsts[r][c].data, exp_c[c][r], kind, f"many {r} {c}")
    return staging


def _same_staging(a, b, kind):
    for side in ("send", "recv"):
        assert len(a[side]) == len(b[side])
        for r, (x, y) in enumerate(zip(a[side], b[side])):
            same(x, y, kind, f"{side} buffer of rank {r}")


def _split_refs(cfg, kind, n, keep, fill_zero, lib, alpha=None):
    """(aos, sources the n-field plan sees, exp[c][r]) of a truncated split:
    the component copies, reference-scaled if ``alpha``, masked by numpy and
    placed by the oracle."""
    ssz = KINDS[kind][1]
    aos, comps, _ = split_case(cfg, ssz, n, lib)
    if alpha is not None:
        comps = [[scale_bytes(x, kind, alpha) for x in row] for row in comps]
    return aos, comps, expected_keep(comps, cfg, ssz, keep, lib, fill_zero,
                                     SENT)


def _join_refs(cfg, kind, n, keep, fill_zero, lib, alpha=None):
    """(fields, exp_c[c][r], exp[r]) of a truncated join; ``exp_c`` is what
    the UNSCALED n-field keep plan delivers (its staging is the join's)."""
    ssz = KINDS[kind][1]
    fields, _, _ = join_case(cfg, ssz, n, lib)
    plain_c = expected_keep(fields, cfg, ssz, keep, lib, fill_zero, SENT)
    exp_c = plain_c
    if alpha is not None:
        scaled = [[scale_bytes(x, kind, alpha) for x in row]
                  for row in fields]
        exp_c = expected_keep(scaled, cfg, ssz, keep, lib, fill_zero, SENT)
    nr = math.prod(cfg[1])
    exp = [interleave([exp_c[c][r] for c in range(n)], ssz)
           for r in range(nr)]
    return fields, plain_c, exp


CASES = [(ci, name, kind) for ci in range(len(CONFIGS))
         for name in KEEP_NAMES for kind in KIND_IDS]


def _case_id(v):
    return f"{_ids(CONFIGS[v[0]])}-{v[1]}-{v[2]}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_split_sim_keep_vs_masked_oracle_and_staging(case, oracle_lib_path):
    ci, name, kind = case
    cfg = CONFIGS[ci]
    keep = cfg_keep_sets(cfg)[name]
    Pi, Po, nr, extra = _pencils(cfg)
    for n in (2, 3, 4):
        for fill in ("zero", None):
            aos, comps, exp = _split_refs(cfg, kind, n, keep, fill == "zero",
                                          oracle_lib_path)
            srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
            dsts = [[_sentinel(Po, r, len(exp[c][r]), kind, extra)
                     for c in range(n)] for r in range(nr)]
            staging = {}
            run_transpose_sim_split(dsts, srcs, staging_out=staging,
                                    keep=keep, fill=fill)
            for r in range(nr):
                for c in range(n):
                    same(dsts[r][c].data, exp[c][r], kind, (n, fill, r, c))
                assert srcs[r].data.tobytes() == aos[r].tobytes()
            _same_staging(staging, _many_staging(cfg, kind, comps, exp, keep,
                                                 fill), kind)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_join_sim_keep_vs_masked_oracle_and_staging(case, oracle_lib_path):
    ci, name, kind = case
    cfg = CONFIGS[ci]
    keep = cfg_keep_sets(cfg)[name]
    Pi, Po, nr, extra = _pencils(cfg)
    for n in (2, 3, 4):
        for fill in ("zero", None):
            fields, exp_c, exp = _join_refs(cfg, kind, n, keep,
                                            fill == "zero", oracle_lib_path)
            srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
                    for r in range(nr)]
            dsts = [_sentinel(Po, r, len(exp[r]), kind, extra, (n,))
                    for r in range(nr)]
            staging = {}
            run_transpose_sim_join(dsts, srcs, staging_out=staging, keep=keep,
                                   fill=fill)
            for r in range(nr):
                same(dsts[r].data, exp[r], kind, (n, fill, r))
            _same_staging(staging, _many_staging(cfg, kind, fields, exp_c,
                                                 keep, fill), kind)


SCALED = [(ci, name, kind, SCALES[(ci + i + k) % 3])
          for ci in range(len(CONFIGS))
          for i, name in enumerate(["inside", "two_dims", "two_ranges"])
          for k, kind in enumerate(KIND_IDS)]


@pytest.mark.parametrize("case", SCALED,
                         ids=lambda v: f"{_case_id(v)}-{v[3]:.3g}")
def test_scaled_sim_keep_is_the_mask_of_the_scaled_input(case,
                                                         oracle_lib_path):
    """Kept scalars are multiplied once; outside K the result is +0 whatever
    the sign of alpha (a -2 would make -0 of a masked zero)."""
    ci, name, kind, alpha = case
    cfg = CONFIGS[ci]
    keep = cfg_keep_sets(cfg)[name]
    Pi, Po, nr, extra = _pencils(cfg)
    n = 2 + ci % 3
    # split: staging carries the scaled kept scalars
    aos, scaled, exp = _split_refs(cfg, kind, n, keep, True, oracle_lib_path,
                                   alpha)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    dsts = [[_sentinel(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging, keep=keep,
                            scale=alpha)
    for r in range(nr):
        for c in range(n):
            same(dsts[r][c].data, exp[c][r], kind, ("split", r, c))
    _same_staging(staging, _many_staging(cfg, kind, scaled, exp, keep,
                                         "zero"), kind)
    # join: staging carries the unscaled kept scalars
    fields, plain_c, exp = _join_refs(cfg, kind, n, keep, True,
                                      oracle_lib_path, alpha)
    srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_sentinel(Po, r, len(exp[r]), kind, extra, (n,))
            for r in range(nr)]
    staging = {}
    run_transpose_sim_join(dsts, srcs, staging_out=staging, keep=keep,
                           scale=alpha)
    for r in range(nr):
        same(dsts[r].data, exp[r], kind, ("join", r))
    _same_staging(staging, _many_staging(cfg, kind, fields, plain_c, keep,
                                         "zero"), kind)


def test_minus_two_leaves_plus_zero_outside_the_keep_set(oracle_lib_path):
    cfg, kind, n = CONFIGS[0], "f64", 2
    keep = cfg_keep_sets(cfg)["two_dims"]
    Pi, Po, nr, extra = _pencils(cfg)
    fields, _, exp = _join_refs(cfg, kind, n, keep, True, oracle_lib_path,
                                -2.0)
    srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_sentinel(Po, r, len(exp[r]), kind, extra, (n,))
            for r in range(nr)]
    run_transpose_sim_join(dsts, srcs, keep=keep, scale=-2.0)
    from keep_util import parent_mask
    outside = 0
    for r in range(nr):
        got = dsts[r].data.view(np.uint64).reshape(-1, n)
        out = ~parent_mask(cfg, keep, r, 1)
        assert not got[out].any()        # all bits zero: +0, never -0
        outside += int(out.sum())
    assert outside > 0


# ---- peers: one side of the hop is the ordinary n-field keep plan ---------

@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
@pytest.mark.parametrize("name", ["inside", "two_dims"])
def test_ordinary_keep_unpack_faces_a_truncated_split_pack(cfg, name,
                                                           oracle_lib_path):
    kind, n = "f64", 3
    keep = cfg_keep_sets(cfg)[name]
    Pi, Po, nr, extra = _pencils(cfg)
    aos, comps, exp = _split_refs(cfg, kind, n, keep, True, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    dsts = [[_sentinel(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging, keep=keep,
                            stages=("pack", "exchange", "local"))
    # the ordinary unpack: the recv buffers of a run whose sources are the
    # component copies must be the same bytes, and its unpack delivers
    ref = _many_staging(cfg, kind, comps, exp, keep, "zero")
    _same_staging(staging, ref, kind)
    from pencilarrays_amd.copyexec import apply_copy
    from pencilarrays_amd.plan import build_plan, stage_descs
    for r in range(nr):
        plan = build_plan(Pi, Po, r, extra, keep=keep)
        for c in range(n):
            for _, d in stage_descs(plan, n, c, 2):
                apply_copy(d, staging["recv"][r], dsts[r][c].data)
            same(dsts[r][c].data, exp[c][r], kind, (r, c))


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
@pytest.mark.parametrize("name", ["inside", "two_dims"])
def test_truncated_join_unpack_faces_an_ordinary_keep_pack(cfg, name,
                                                           oracle_lib_path):
    kind, n = "f64", 3
    keep = cfg_keep_sets(cfg)[name]
    Pi, Po, nr, extra = _pencils(cfg)
    fields, exp_c, exp = _join_refs(cfg, kind, n, keep, True, oracle_lib_path)
    staging = _many_staging(cfg, kind, fields, exp_c, keep, "zero")
    srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_sentinel(Po, r, len(exp[r]), kind, extra, (n,))
            for r in range(nr)]
    run_transpose_sim_join(dsts, srcs, stages=("local", "unpack"),
                           staging_in=staging, keep=keep)
    for r in range(nr):
        same(dsts[r].data, exp[r], kind, r)


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5], CONFIGS[9]], ids=_ids)
def test_split_then_join_is_the_identity_on_the_keep_set(cfg,
                                                         oracle_lib_path):
    kind, n = "f64", 3
    ssz = 8
    keep = cfg_keep_sets(cfg)["two_dims"]
    dims, pdims, di, pi, do, po, extra = cfg
    back_cfg = (dims, pdims, do, po, di, pi, extra)
    Pi, Po, nr, _ = _pencils(cfg)
    aos, comps, exp = _split_refs(cfg, kind, n, keep, True, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    mids = [[_sentinel(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    run_transpose_sim_split(mids, srcs, keep=keep)
    back = [_sentinel(Pi, r, len(aos[r]), kind, extra, (n,))
            for r in range(nr)]
    run_transpose_sim_join(back, mids, keep=keep)
    # the masked source: numpy on the keep mask of the input pencil
    from keep_util import parent_mask
    for r in range(nr):
        want = aos[r].reshape(-1, n * ssz).copy()
        want[~parent_mask(cfg, keep, r, 0)] = 0
        same(back[r].data, want.reshape(-1), kind, r)
    assert back_cfg[2] == do


# ---- the classes on numpy arrays -------------------------------------------

@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("fill", ["zero", None])
def test_classes_world1_numpy_keep(permuted, fill, oracle_lib_path):
    kind, n, ssz = "f64", 3, 8
    cfg = ((13, 11, 7), (1, 1), (1, 2), ID3, (0, 2),
           (1, 2, 0) if permuted else ID3, ())
    keep = [(9, 0), (4, 3), None]
    kfull = [(9, 0), (4, 3), (7, 0)]
    Pi, Po, _, extra = _pencils(cfg)
    aos, comps, exp = _split_refs(cfg, kind, n, kfull, fill == "zero",
                                  oracle_lib_path, 0.5)
    src = _arr(Pi, 0, aos[0], kind, extra, (n,))
    dsts = [_sentinel(Po, 0, len(exp[c][0]), kind, extra) for c in range(n)]
    t = SplitTransposition(dsts, src, scale=0.5, keep=keep, fill=fill)
    assert t.grouped and t.execute() is t.dests
    for c in range(n):
        same(dsts[c].data, exp[c][0], kind, c)
    fields, _, expj = _join_refs(cfg, kind, n, kfull, fill == "zero",
                                 oracle_lib_path)
    srcs = [_arr(Pi, 0, fields[c][0], kind, extra) for c in range(n)]
    dst = _sentinel(Po, 0, len(expj[0]), kind, extra, (n,))
    assert transpose_join_into(dst, srcs, keep=keep, fill=fill) is dst
    same(dst.data, expj[0], kind, "join")
    again = [_sentinel(Po, 0, len(exp[c][0]), kind, extra) for c in range(n)]
    transpose_split_into(again, src, scale=0.5, keep=keep, fill=fill)
    for c in range(n):
        same(again[c].data, exp[c][0], kind, c)


def test_python_value_errors_of_keep_and_grouped():
    topo = Topology((1, 1))
    dims = (6, 5, 4)
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    a = PencilArray.empty(Pi, 0, np.float64, elem_dims=(3,))
    fs = [PencilArray.empty(Po, 0, np.float64) for _ in range(3)]
    keep = [(4, 0), None, None]
    for make in (lambda **kw: SplitTransposition(fs, a, **kw),
                 lambda **kw: JoinTransposition(
                     PencilArray.empty(Po, 0, np.float64, elem_dims=(3,)),
                     [PencilArray.empty(Pi, 0, np.float64) for _ in range(3)],
                     **kw)):
        assert make().grouped is False and make().keep is None
        assert make(grouped=True).grouped is True
        assert make(keep=keep).grouped is True
        assert make(keep=keep, grouped=True).grouped is True
        with pytest.raises(ValueError, match="grouped=False"):
            make(keep=keep, grouped=False)
        # Transposition's validation of keep and fill
        with pytest.raises(ValueError, match="fill must be"):
            make(keep=keep, fill="ones")
        with pytest.raises(ValueError):
            make(keep=[(4, 0), None])
        with pytest.raises(ValueError):
            make(keep=[(4, 3), None, None])


def _gloo_worker(rank, world, port, lib):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        kind, n = "f64", 3
        cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        # rank 1 owns x >= 8 after the hop and nothing of it is kept: the
        # message 0 -> 1 and 1 -> 1's local block are empty
        keep = [(8, 0), (14, 0), None]
        kfull = [(8, 0), (14, 0), (41, 0)]
        Pi, Po, _, extra = _pencils(cfg)
        aos, _, exp = _split_refs(cfg, kind, n, kfull, True, lib)
        src = _arr(Pi, rank, aos[rank], kind, extra, (n,))
        dsts = [_sentinel(Po, rank, len(exp[c][rank]), kind, extra)
                for c in range(n)]
        transpose_split_into(dsts, src, keep=keep)
        for c in range(n):
            same(dsts[c].data, exp[c][rank], kind, (rank, c))
        fields, _, expj = _join_refs(cfg, kind, n, kfull, True, lib, 0.5)
        srcs = [_arr(Pi, rank, fields[c][rank], kind, extra)
                for c in range(n)]
        dst = _sentinel(Po, rank, len(expj[rank]), kind, extra, (n,))
        transpose_join_into(dst, srcs, keep=keep, scale=0.5)
        same(dst.data, expj[rank], kind, rank)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2_with_a_zero_byte_message(oracle_lib_path):
    from keep_util import pair_counts
    cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    c = pair_counts(cfg, [(8, 0), (14, 0), (41, 0)])
    assert c[0][1] == 0 and c[1][0] > 0   # one direction carries nothing
    mp.spawn(_gloo_worker, args=(2, 31500 + os.getpid() % 2000,
                                 oracle_lib_path), nprocs=2, join=True)


# ---- the native plan flag, host only ----------------------------------------

# both messages of rank 0 and its local block keep something
KEEP3 = ((6, 0), (5, 0), (4, 0))


def _slab(**kw):
    topo = Topology((2,))
    dims = (8, 6, 4)
    return native.NativePlan(Pencil(topo, dims, (1,)),
                             Pencil(topo, dims, (0,), permute=(1, 0, 2)), 0,
                             kw.pop("esz", 8), (), **kw)


def _stage_calls(p, n=3):
    ptrs = [4096 * (c + 2) for c in range(n)]
    F = native.SCALAR_F64
    return [lambda: p.pack_split(n, 4096),
            lambda: p.local_split(4096, ptrs),
            lambda: p.local_join(ptrs, 4096),
            lambda: p.unpack_join(n, 4096),
            lambda: p.execute_split(4096, ptrs),
            lambda: p.execute_join(ptrs, 4096),
            lambda: p.pack_split_scaled(n, F, 0.5, 4096),
            lambda: p.local_split_scaled(F, 0.5, 4096, ptrs),
            lambda: p.local_join_scaled(F, 0.5, ptrs, 4096),
            lambda: p.unpack_join_scaled(n, F, 0.5, 4096),
            lambda: p.execute_split_scaled(F, 0.5, 4096, ptrs),
            lambda: p.execute_join_scaled(F, 0.5, ptrs, 4096)]


def test_flag_value_and_query():
    assert native.PLAN_GROUP_SOA == 4
    assert _slab().group_soa() is False
    assert _slab(group_soa=True).group_soa() is True
    assert _slab(group_soa=True, keep=KEEP3).group_soa() is True
    assert _slab(group_soa=True, esz=4).group_soa() is True
    assert _slab(group_soa=True, esz=16).group_soa() is True


def test_unflagged_keep_plan_is_still_refused_and_flagged_is_accepted():
    p = _slab(keep=KEEP3)
    for call in _stage_calls(p):
        with pytest.raises(RuntimeError, match="cannot run on a keep plan"):
            call()
    # the flagged keep plan gets past the plan checks: the next refusal is
    # the missing staging, which needs no device
    q = _slab(keep=KEEP3, group_soa=True)
    for call in _stage_calls(q):
        with pytest.raises(RuntimeError, match="pa_plan_buffer_sizes_many"):
            call()


def _scaled_plan():
    p = _slab(group_soa=True)
    p.set_scale(native.SCALAR_F64, 0.5)
    return p


@pytest.mark.parametrize("make,msg,on", [
    (lambda: _slab(group_soa=True, aliased=True),
     "PA_PLAN_ALIASED plan: the two sides have different element sizes", 0),
    (lambda: _slab(group_soa=True, wire=native.WIRE_F64_F32), "wire plan", 0),
    (lambda: _slab(group_soa=True, ncomp=3),
     "needs a scalar plan: this one has ncomp = 3", 0),
    (lambda: _slab(group_soa=True, esz=2), "invalid scalar_size 2", 0),
    (lambda: _slab(group_soa=True, aliased=True, keep=KEEP3),
     "PA_PLAN_ALIASED plan", 0),
    (_scaled_plan, "plan with a scale set", 1),
], ids=["aliased", "wire", "composite", "int16", "aliased-keep", "scale"])
def test_flag_is_ignored_where_it_does_not_apply(make, msg, on):
    p = make()
    assert p.group_soa() is bool(on)
    for call in _stage_calls(p):
        with pytest.raises(RuntimeError, match=msg):
            call()
    with pytest.raises(RuntimeError, match=msg):
        p.stage_launches_soa(3, native.SOA_SPLIT, native.STAGE_PACK)


@pytest.mark.parametrize("keep", [None, KEEP3, ((8, 0), (6, 0), (4, 0))],
                         ids=["ordinary", "keep", "fullkeep"])
def test_flag_changes_nothing_else_about_a_plan(keep):
    a, b = _slab(keep=keep), _slab(keep=keep, group_soa=True)
    for n in (1, 3):
        assert a.buffer_sizes_many(n) == b.buffer_sizes_many(n)
        for k in range(2):
            assert a.peer_message(n, k) == b.peer_message(n, k)
        for stage in (native.STAGE_PACK, native.STAGE_LOCAL,
                      native.STAGE_UNPACK):
            assert a.stage_launches(n, stage) == b.stage_launches(n, stage)
    assert a.buffer_sizes() == b.buffer_sizes()
    if keep is None:
        for which in (0, 1, 2):
            for k in range(2):
                assert a.copydesc(which, k) == b.copydesc(which, k)
                assert a.copydesc_many(3, 1, which, k) == \
                    b.copydesc_many(3, 1, which, k)
    else:
        assert a.nfill() == b.nfill()
        for i in range(a.nfill()):
            assert a.filldesc(i) == b.filldesc(i)
        for which in (0, 1, 2):
            for k in range(2):
                assert a.nsub(which, k) == b.nsub(which, k)
                for s in range(a.nsub(which, k)):
                    assert a.copydesc_sub(3, 1, which, k, s) == \
                        b.copydesc_sub(3, 1, which, k, s)


def test_full_keep_set_equals_the_flagged_ordinary_plan():
    full = _slab(keep=((8, 0), (6, 0), (4, 0)), group_soa=True)
    ordinary = _slab(group_soa=True)
    assert full.nfill() == 0
    assert full.buffer_sizes_many(3) == ordinary.buffer_sizes_many(3)
    for d, stages in ((native.SOA_SPLIT, (native.STAGE_PACK,
                                          native.STAGE_LOCAL)),
                      (native.SOA_JOIN, (native.STAGE_LOCAL,
                                         native.STAGE_UNPACK))):
        for stage in stages:
            rows = full.stage_launches_soa(3, d, stage)
            assert rows == ordinary.stage_launches_soa(3, d, stage)
            assert all(r.kind != native.KERNEL_FILL for r in rows)
    for which in (0, 1, 2):
        for k in range(2):
            assert full.nsub(which, k) == (
                1 if ordinary.copydesc(which, k) is not None else 0)
            if full.nsub(which, k):
                assert full.copydesc_sub(1, 0, which, k, 0) == \
                    ordinary.copydesc(which, k)
