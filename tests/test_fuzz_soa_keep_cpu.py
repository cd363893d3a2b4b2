"""Host counterpart of test_gpu_fuzz_soa_keep.py: 60 seeded trials (12 of
each flavour) of the mirror, run_transpose_sim_split / _join with ``keep``,
against the C oracle on the numpy-masked and reference-scaled input, staging
against run_transpose_sim_many on the component copies."""

from __future__ import annotations

import numpy as np
import pytest

from keep_util import expected_keep
from many_util import expected_dests
from soa_keep_fuzz_util import FLAVOURS, draw, trial_ids
from soa_scale_util import KINDS, same, scale_bytes
from soa_util import interleave, join_case, split_case
from pencilarrays_amd import (
    Pencil, PencilArray, Topology, native, run_transpose_sim_join,
    run_transpose_sim_many, run_transpose_sim_split,
)

SENT = 0xAB
TRIALS = 60 // len(FLAVOURS)


def _arr(P, r, raw, kind, extra, elem_dims=()):
    return PencilArray(P, r, raw.view(KINDS[kind][0]).copy(), extra,
                       elem_dims)


def _sentinel(P, r, nbytes, kind, extra, elem_dims=()):
    raw = np.full(nbytes, SENT, dtype=np.uint8)
    return PencilArray(P, r, raw.view(KINDS[kind][0]), extra, elem_dims)


@pytest.mark.parametrize("flavour,index", trial_ids(TRIALS),
                         ids=lambda v: str(v))
def test_fuzz_mirror(flavour, index, oracle_lib_path):
    cfg, kind, n, direction, keep, fill, alpha = draw(flavour, index)
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr, ssz = topo.nranks, KINDS[kind][1]
    split = direction == native.SOA_SPLIT
    fz = fill == native.FILL_ZERO
    pyfill = "zero" if fz else None
    if split:
        aos, comps, _ = split_case(cfg, ssz, n, oracle_lib_path)
    else:
        comps, _, _ = join_case(cfg, ssz, n, oracle_lib_path)
    scaled = comps if alpha is None else \
        [[scale_bytes(x, kind, alpha) for x in row] for row in comps]

    def expect(parents):
        if keep is None:
            return expected_dests(parents, cfg, ssz, oracle_lib_path)
        return expected_keep(parents, cfg, ssz, keep, oracle_lib_path, fz,
                             SENT)
    exp_c = expect(scaled)
    staging = {}
    if split:
        srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
        dsts = [[_sentinel(Po, r, len(exp_c[c][r]), kind, extra)
                 for c in range(n)] for r in range(nr)]
        run_transpose_sim_split(dsts, srcs, staging_out=staging, scale=alpha,
                                keep=keep, fill=pyfill)
        for r in range(nr):
            for c in range(n):
                same(dsts[r][c].data, exp_c[c][r], kind, (r, c))
        staged = scaled
    else:
        srcs = [[_arr(Pi, r, comps[c][r], kind, extra) for c in range(n)]
                for r in range(nr)]
        exp = [interleave([exp_c[c][r] for c in range(n)], ssz)
               for r in range(nr)]
        dsts = [_sentinel(Po, r, len(exp[r]), kind, extra, (n,))
                for r in range(nr)]
        run_transpose_sim_join(dsts, srcs, staging_out=staging, scale=alpha,
                               keep=keep, fill=pyfill)
        for r in range(nr):
            same(dsts[r].data, exp[r], kind, r)
        staged = comps
    # staging: the n-field run on the (scaled, for a split) component copies
    msrc = [[_arr(Pi, r, staged[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    mdst = [[_sentinel(Po, r, len(exp_c[c][r]), kind, extra)
             for c in range(n)] for r in range(nr)]
    ref = {}
    run_transpose_sim_many(mdst, msrc, staging_out=ref, keep=keep,
                           fill=pyfill)
    for side in ("send", "recv"):
        for r in range(nr):
            same(staging[side][r], ref[side][r], kind, (side, r))
