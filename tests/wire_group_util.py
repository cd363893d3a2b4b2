"""Helpers of the grouped converting-kernel tests (PA_PLAN_GROUP_CVT).

Expected launch rows never come from the flagged plan: the UNFLAGGED plan's
``stage_launches`` rows give one ``(kind, workgroups)`` per non-empty
descriptor in launch order, ``copy_kernel_kind_wire`` per descriptor gives the
scalars per access, and ``partition`` groups them by signature in
first-appearance order.  Expected values are the C oracle on the
reference-rounded input.  The device part runs all ranks of a config on one
GPU through the stage API, flagged and unflagged on the same inputs."""

from __future__ import annotations

import math

import numpy as np

from pencilarrays_amd import Pencil, Topology, build_plan, native
from wire_util import (
    NARROW, PAIRS, ROUND, WIDEN, assert_same, oracle, ref_round,
)

LIN, TILE, GEN = (native.KERNEL_CVT_LINEAR, native.KERNEL_CVT_TILE,
                  native.KERNEL_CVT_GENERIC)
STAGES = (native.STAGE_PACK, native.STAGE_LOCAL, native.STAGE_UNPACK)
A = 256  # the address the engine assumes for a pointer it is not given

# the op of each `which` of pa_plan_copydesc
WHICH_OP = {0: ROUND, 1: NARROW, 2: WIDEN, 3: NARROW, 4: WIDEN}


def pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po))


def wire_plan(cfg, r, pair, nc, aliased=False, **kw):
    Pi, Po = pencils(cfg)
    stored = np.dtype(PAIRS[pair][0]).itemsize
    return native.NativePlan(Pi, Po, r, stored, cfg[6], aliased=aliased,
                             ncomp=nc, wire=PAIRS[pair][2], **kw)


def stage_order(py, n):
    """``(stage, f, which, k)`` of every descriptor the three stage calls of
    an ordinary-shaped plan launch, in launch order."""
    out = []
    for f in range(n):
        for b in py.peers:
            if b.pack is not None:
                out.append((native.STAGE_PACK, f, 1, b.peer_k))
        if py.self_pack is not None:
            out.append((native.STAGE_PACK, f, 3, 0))
    for f in range(n):
        if py.local is not None:
            out.append((native.STAGE_LOCAL, f, 0, 0))
        if py.self_unpack is not None:
            out.append((native.STAGE_LOCAL, f, 4, 0))
    for f in range(n):
        for b in py.peers:
            if b.unpack is not None:
                out.append((native.STAGE_UNPACK, f, 2, b.peer_k))
    return out


def partition(per_desc):
    """``[(kind, op, V, workgroups)]`` in launch order -> the rows of a
    flagged plan: linear entries of one (op, V) and tile entries of one op
    share a grouped row, in first-appearance order; generic entries stay
    alone."""
    rows = []
    for kind, op, vec, wg in per_desc:
        sig = {LIN: (LIN, op, vec), TILE: (TILE, op)}.get(kind)
        hit = next((r for r in rows if sig is not None and r[0] == sig), None)
        if hit is not None:
            hit[2] += 1
            hit[3] += wg
        else:
            rows.append([sig, kind, 1, wg])
    return [native.StageLaunch(kind, sig is not None, ne, wg)
            for sig, kind, ne, wg in rows]


def expected_rows(plain, py, n, pair, nc, sp=None, dp=None, send=A, recv=A):
    """Per stage, the rows a flagged plan must report, from the unflagged
    plan ``plain`` and the selection query, with the same pointers."""
    code = PAIRS[pair][2]
    sp = sp or [A] * n
    dp = dp or [A] * n
    per = {s: [] for s in STAGES}
    for stage, f, which, k in stage_order(py, n):
        src = {0: sp[f], 1: sp[f], 3: sp[f], 2: recv, 4: recv}[which]
        dst = {0: dp[f], 1: send, 3: recv, 2: dp[f], 4: dp[f]}[which]
        kk = native.copy_kernel_kind_wire(
            plain.copydesc_many(n, f, which, k), code, WHICH_OP[which], nc,
            src, dst)
        if kk.kind != native.KERNEL_NONE:
            per[stage].append((kk.kind, WHICH_OP[which], kk.vec))
    out = {}
    for stage in STAGES:
        rows = plain.stage_launches(n, stage, sp, dp)
        assert all(not l.grouped and l.entries == 1 for l in rows), rows
        assert [l.kind for l in rows] == [k for k, _, _ in per[stage]], \
            (stage, rows, per[stage])
        out[stage] = partition([(k, op, v, l.workgroups)
                                for (k, op, v), l in zip(per[stage], rows)])
    return out


def flagged_rows(plan, n, sp=None, dp=None):
    return {s: plan.stage_launches(n, s, sp, dp) for s in STAGES}


def parents_of(cfg, pair, nc, n, values, oracle_lib_path):
    """``parents[f][r]``: stored scalars of field ``f`` on rank ``r``, drawn
    by ``values(count, seed)``."""
    dims, pdims, di, _, _, _, extra = cfg
    orc = oracle(oracle_lib_path)
    return [[values(orc.local_len(dims, pdims, di, extra, r) * nc,
                    0x6C0 + 131 * f + r)
             for r in range(math.prod(pdims))] for f in range(n)]


def expected_of(cfg, pair, nc, parents, oracle_lib_path):
    """``exp[f][r]``: the C oracle, moving opaque elements of the stored
    size, on the reference-rounded parents (wire_util.expected_rounded for
    any component count)."""
    dims, pdims, di, pi, do, po, extra = cfg
    stored = np.dtype(PAIRS[pair][0])
    orc = oracle(oracle_lib_path)
    return [[o.view(stored) for o in orc.transpose_all(
        [ref_round(p, pair) for p in row], dims, pdims, di, pi, do, po, extra,
        stored.itemsize * nc)] for row in parents]


def _run(cfg, pair, nc, parents, exp, group, aliased, lead, rows_hook):
    """One pass of every rank through pack_many -> slice copies ->
    local_many -> unpack_many.  Returns the bytes of every destination
    allocation and staging buffer, guards included."""
    import torch
    from wire_gpu_util import GUARD, SENT, dev, sentinel

    n, nr = len(parents), len(parents[0])
    stored = np.dtype(PAIRS[pair][0])
    isz = stored.itemsize
    Pi, Po = pencils(cfg)
    pyplans = [build_plan(Pi, Po, r, cfg[6], aliased=aliased)
               for r in range(nr)]
    plans = [wire_plan(cfg, r, pair, nc, aliased, group_cvt=group)
             for r in range(nr)]
    assert all(p.group_cvt() == group for p in plans)

    def lead_b(f):
        return lead.get(f, 0) * isz

    s_all = [[torch.cat([torch.full((lead_b(f),), 0x5C, dtype=torch.uint8,
                                    device="cuda:0"),
                         dev(parents[f][r]) if parents[f][r].size
                         else sentinel(0)])
              for f in range(n)] for r in range(nr)]
    d_all = [[sentinel(lead_b(f) + exp[f][r].nbytes) for f in range(n)]
             for r in range(nr)]
    sp = [[s_all[r][f].data_ptr() + lead_b(f) for f in range(n)]
          for r in range(nr)]
    dp = [[d_all[r][f].data_ptr() + lead_b(f) for f in range(n)]
          for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [sentinel(s) for s, _ in sizes]
    recvs = [sentinel(rb) for _, rb in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())

    # launch rows through the query, real pointers, before anything runs
    if group:
        for r, p in enumerate(plans):
            plain = wire_plan(cfg, r, pair, nc, aliased)
            plain.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
            want = expected_rows(plain, pyplans[r], n, pair, nc, sp[r], dp[r],
                                 sends[r].data_ptr(), recvs[r].data_ptr())
            got = flagged_rows(p, n, sp[r], dp[r])
            assert got == want, (r, got, want)
            if rows_hook is not None:
                rows_hook(r, got)
            plain.set_buffers(0, 0)

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        p.pack_many(sp[r], stream)
    for r, p in enumerate(plans):
        for blk in pyplans[r].peers:
            if blk.peer_k == pyplans[r].my_k:
                continue
            so, sn, _, _ = p.peer_message(n, blk.peer_k)
            _, _, ro, rn = plans[blk.global_rank].peer_message(
                n, pyplans[r].my_k)
            assert sn == rn
            if sn:
                recvs[blk.global_rank][ro:ro + rn] = sends[r][so:so + sn]
    for r, p in enumerate(plans):
        p.local_many(sp[r], dp[r], stream)
        p.unpack_many(dp[r], stream)
    torch.cuda.synchronize()

    out = {"dst": [[t.cpu().numpy() for t in row] for row in d_all],
           "send": [t.cpu().numpy() for t in sends],
           "recv": [t.cpu().numpy() for t in recvs]}
    for r in range(nr):
        for f in range(n):
            got, lb, nb = out["dst"][r][f], lead_b(f), exp[f][r].nbytes
            assert (got[:lb] == SENT).all(), f"rank {r} field {f} lead"
            assert_same(got[lb:lb + nb].view(stored), exp[f][r],
                        f"rank {r} field {f} group={group}")
            assert (got[lb + nb:] == SENT).all(), f"rank {r} field {f} guard"
            assert got.size == lb + nb + GUARD
        for name, nbytes in (("send", sizes[r][0]), ("recv", sizes[r][1])):
            assert (out[name][r][nbytes:] == SENT).all(), \
                f"rank {r} {name} guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)
    return out


def run_stage_sim_grouped(cfg, pair, nc, parents, exp, aliased=False,
                          lead=None, rows_hook=None):
    """All ranks of ``cfg`` on one GPU through the stage API, once with
    unflagged and once with flagged wire plans on the same inputs.  Asserts
    the flagged rows against ``expected_rows`` (and ``rows_hook(rank,
    rows_by_stage)``), every destination against ``exp`` and every guard in
    both runs, and that the two runs leave byte-identical destinations and
    staging buffers.  ``lead[f]``: field ``f`` starts that many stored
    scalars into its allocations."""
    lead = lead or {}
    a = _run(cfg, pair, nc, parents, exp, False, aliased, lead, None)
    b = _run(cfg, pair, nc, parents, exp, True, aliased, lead, rows_hook)
    for r in range(len(parents[0])):
        for f in range(len(parents)):
            assert np.array_equal(a["dst"][r][f], b["dst"][r][f]), (r, f)
        for name in ("send", "recv"):
            assert np.array_equal(a[name][r], b[name][r]), (r, name)
