"""Expected launch rows of the split / join stages, shared by the host and
device tests of PA_PLAN_GROUP_SOA.  Nothing here asks the flagged plan: the
descriptors are the Python plan's, the kernel of each comes from
pa_copy_kernel_kind_soa with the pointers the stage uses, the workgroups from
the UNFLAGGED plan's rows, and the grouping rule is restated."""

from __future__ import annotations

import math

from pencilarrays_amd import native
from pencilarrays_amd.plan import stage_descs

PACK, LOCAL, UNPACK = (native.STAGE_PACK, native.STAGE_LOCAL,
                       native.STAGE_UNPACK)
LIN, TILE, GEN, FILL = (native.KERNEL_SOA_LINEAR, native.KERNEL_SOA_TILE,
                        native.KERNEL_SOA_GENERIC, native.KERNEL_FILL)
A = 256      # the address the engine assumes for a pointer it is not given


def _tup(d):
    return (d.dims, d.sstrides, d.soffset, d.dstrides, d.doffset)


def _descs(pl, n, d, stage, ssz, aos, fields, staging=A):
    """[(descriptor, field pointers)] of a split / join stage in the order
    the engine walks them: component 0's descriptor of every sub-block, and
    for a staged block the component slots ``staging + c * count * S``."""
    out = []
    for which, desc in stage_descs(pl, n, 0, {PACK: 0, LOCAL: 1,
                                              UNPACK: 2}[stage]):
        if stage == LOCAL:
            assert which == 0
            out.append((desc, list(fields)))
        else:
            cnt = math.prod(desc.dims)
            out.append((desc, [staging + c * cnt * ssz for c in range(n)]))
    return out


def expected_rows(flat, pl, n, d, stage, ssz, aos=A, fields=None,
                  staging=A):
    """(rows the flagged plan must report, rows the unflagged one must):
    ``flat`` is the UNFLAGGED native plan, whose workgroups are summed;
    ``staging`` the buffer the stage packs into or unpacks from."""
    fields = fields or [A] * n
    unflagged = flat.stage_launches_soa(n, d, stage, aos, fields)
    kinds = []
    for desc, fp in _descs(pl, n, d, stage, ssz, aos, fields, staging):
        k = native.copy_kernel_kind_soa(_tup(desc), ssz, n, d, aos, fp)
        if k.kind != native.KERNEL_NONE:
            kinds.append(k)
    assert [(u.kind, u.grouped, u.entries) for u in unflagged] == \
        [(k.kind, False, 1) for k in kinds], (unflagged, kinds)
    rows = []    # [kind, grouped, entries, workgroups, V]
    for k, u in zip(kinds, unflagged):
        if k.kind == GEN:
            rows.append([GEN, False, 1, u.workgroups, 0])
            continue
        vec = k.vec if k.kind == LIN else 0
        for r in rows:
            if r[1] and r[0] == k.kind and r[4] == vec:
                r[2] += 1
                r[3] += u.workgroups
                break
        else:
            rows.append([k.kind, True, 1, u.workgroups, vec])
    return [tuple(r[:4]) for r in rows], unflagged



def keep_rows(pl, n, d, stage, ssz, aos, fields, staging, nfill):
    """[(kind, grouped, entries)] a flagged KEEP plan must report (there is
    no unflagged plan to take workgroups from: it refuses): the partition of
    the sub-boxes, then the FILL row of the local stage, ``nfill`` being the
    plan's non-empty fill windows."""
    rows = []    # [kind, grouped, entries, V]
    for desc, fp in _descs(pl, n, d, stage, ssz, aos, fields, staging):
        k = native.copy_kernel_kind_soa(_tup(desc), ssz, n, d, aos, fp)
        if k.kind == native.KERNEL_NONE:
            continue
        if k.kind == GEN:
            rows.append([GEN, False, 1, 0])
            continue
        vec = k.vec if k.kind == LIN else 0
        for r in rows:
            if r[1] and r[0] == k.kind and r[3] == vec:
                r[2] += 1
                break
        else:
            rows.append([k.kind, True, 1, vec])
    if stage == LOCAL and nfill:
        rows.append([FILL, True, nfill * (n if d == native.SOA_SPLIT else 1),
                     0])
    return [tuple(r[:3]) for r in rows]
