"""One split / join hop of every rank of a grid on ONE GPU, shared by the
device tests of PA_PLAN_GROUP_SOA and truncated split / join transposes.

Device slice copies at the pa_plan_peer_message ranges stand in for the
exchange.  References never come from the code under test: the placement is
the C oracle per component on the numpy-masked and reference-scaled input,
the staging is the n-field HOST run (run_transpose_sim_many) on the
(scaled, for a split) component copies.  Destinations and staging are
0xAB-filled with 256-byte guards; whole buffers are compared as bit patterns,
NaN for NaN-ness.  Every rank's rows are asserted through the query with the
real pointers before anything is launched."""

from __future__ import annotations

import math

import numpy as np
import torch

from keep_util import expected_keep
from many_util import expected_dests
from soa_group_util import LOCAL, PACK, UNPACK, expected_rows, keep_rows
from soa_scale_util import KINDS, same, scale_bytes
from soa_util import interleave, join_case, split_case
from pencilarrays_amd import (
    Pencil, PencilArray, Topology, build_plan, native, run_transpose_sim_many,
)

GUARD = 256
SENT = 0xAB
DEV = "cuda:0"
SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)


def pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po), topo.nranks, extra)


def exchange(plans, pyplans, n, sends, recvs):
    """The host's exchange: ONE slice copy per peer pair, all n components."""
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


def host_staging(cfg, kind, srcs_c, nbytes_c, keep, fill):
    """send / recv buffers per rank of the n-field HOST run on scalar sources
    ``srcs_c[c][r]`` (bytes)."""
    Pi, Po, nr, extra = pencils(cfg)
    n = len(srcs_c)
    dt = KINDS[kind][0]
    srcs = [[PencilArray(Pi, r, srcs_c[c][r].view(dt).copy(), extra)
             for c in range(n)] for r in range(nr)]
    dsts = [[PencilArray(Po, r, np.zeros(nbytes_c[c][r] // dt.itemsize,
                                         dtype=dt), extra)
             for c in range(n)] for r in range(nr)]
    out = {}
    run_transpose_sim_many(dsts, srcs, staging_out=out, keep=keep,
                           fill="zero" if fill else None)
    return out


def references(cfg, kind, n, direction, lib, keep=None, fill_zero=True,
               alpha=None, seed=None):
    """``(aos or None, fields-side sources, exp_c, exp_aos or None, staged)``:
    ``staged[c][r]`` are the scalar sources whose n-field host run has the
    hop's staging (the scaled copies for a split, the plain ones for a
    join)."""
    ssz = KINDS[kind][1]
    kw = {} if seed is None else {"seed": seed}
    if direction == SPLIT:
        aos, comps, _ = split_case(cfg, ssz, n, lib, **kw)
    else:
        aos = None
        comps, _, _ = join_case(cfg, ssz, n, lib, **kw)
    scaled = comps if alpha is None else \
        [[scale_bytes(x, kind, alpha) for x in row] for row in comps]
    if keep is None:
        exp_c = expected_dests(scaled, cfg, ssz, lib)
    else:
        exp_c = expected_keep(scaled, cfg, ssz, keep, lib, fill_zero, SENT)
    nr = math.prod(cfg[1])
    exp_aos = None
    if direction == JOIN:
        exp_aos = [interleave([exp_c[c][r] for c in range(n)], ssz)
                   for r in range(nr)]
    staged = scaled if direction == SPLIT else comps
    return aos, comps, exp_c, exp_aos, staged


def run_hop(cfg, kind, n, direction, lib, group=True, keep=None,
            fill=native.FILL_ZERO, alpha=None, check=None, seed=None,
            assert_rows=True, refs=None):
    """All ranks of ``cfg`` through the split or join stages (scaled calls if
    ``alpha``) and the ordinary n-field stages of the other side.  Asserts
    destinations, staging and guards; returns ``(dest bytes per rank, send,
    recv)`` as numpy arrays, guards included, for byte comparisons between
    runs.  ``check(plan, pyplan, aos_ptr, field_ptrs, send_ptr, recv_ptr)``
    runs per rank before any launch."""
    dt, ssz, _, code = KINDS[kind]
    split = direction == SPLIT
    Pi, Po, nr, extra = pencils(cfg)
    if refs is None:
        refs = references(cfg, kind, n, direction, lib, keep,
                          fill == native.FILL_ZERO, alpha, seed)
    aos, comps, exp_c, exp_aos, staged = refs
    ref = host_staging(cfg, kind, staged,
                       [[len(x) for x in row] for row in exp_c], keep, fill)

    pyplans = [build_plan(Pi, Po, r, extra, keep=keep,
                          fill="zero" if fill else None) for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, ssz, extra, keep=keep, fill=fill,
                               group_soa=group) for r in range(nr)]
    flats = [None if keep is not None else
             native.NativePlan(Pi, Po, r, ssz, extra) for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [sentinel(s) for s, _ in sizes]
    recvs = [sentinel(rb) for _, rb in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())

    def up(x):
        return dev(x) if len(x) else sentinel(0)

    if split:
        a_t = [up(aos[r]) for r in range(nr)]
        f_t = [[sentinel(len(exp_c[c][r])) for c in range(n)]
               for r in range(nr)]
    else:
        a_t = [sentinel(len(exp_aos[r])) for r in range(nr)]
        f_t = [[up(comps[c][r]) for c in range(n)] for r in range(nr)]
    ap = [t.data_ptr() for t in a_t]
    fp = [[t.data_ptr() for t in row] for row in f_t]

    for r, p in enumerate(plans):
        if assert_rows and group:
            stages = ((PACK, sends[r]), (LOCAL, None)) if split else \
                ((LOCAL, None), (UNPACK, recvs[r]))
            for stage, stg in stages:
                sptr = stg.data_ptr() if stg is not None else 0
                got = p.stage_launches_soa(n, direction, stage, ap[r], fp[r])
                if keep is None:
                    want, _ = expected_rows(flats[r], pyplans[r], n,
                                            direction, stage, ssz, ap[r],
                                            fp[r], sptr)
                    assert [tuple(g) for g in got] == want, (r, stage)
                else:
                    want = keep_rows(pyplans[r], n, direction, stage, ssz,
                                     ap[r], fp[r], sptr,
                                     sum(1 for f in pyplans[r].fills
                                         if f.nelem))
                    assert [tuple(g)[:3] for g in got] == want, (r, stage)
        if check is not None:
            check(p, pyplans[r], ap[r], fp[r], sends[r].data_ptr(),
                  recvs[r].data_ptr())

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        if not split:
            p.pack_many(fp[r], stream)
        elif alpha is None:
            p.pack_split(n, ap[r], stream)
        else:
            p.pack_split_scaled(n, code, alpha, ap[r], stream)
    exchange(plans, pyplans, n, sends, recvs)
    for r, p in enumerate(plans):
        if split:
            if alpha is None:
                p.local_split(ap[r], fp[r], stream)
            else:
                p.local_split_scaled(code, alpha, ap[r], fp[r], stream)
            p.unpack_many(fp[r], stream)
        elif alpha is None:
            p.local_join(fp[r], ap[r], stream)
            p.unpack_join(n, ap[r], stream)
        else:
            p.local_join_scaled(code, alpha, fp[r], ap[r], stream)
            p.unpack_join_scaled(n, code, alpha, ap[r], stream)
    torch.cuda.synchronize()

    outs, so, ro = [], [], []
    for r in range(nr):
        if split:
            row = []
            for c in range(n):
                nb = len(exp_c[c][r])
                got = f_t[r][c].cpu().numpy()
                same(got[:nb], exp_c[c][r], kind, f"rank {r} field {c}")
                assert (got[nb:] == SENT).all(), f"rank {r} field {c} guard"
                row.append(got)
            outs.append(row)
        else:
            nb = len(exp_aos[r])
            got = a_t[r].cpu().numpy()
            same(got[:nb], exp_aos[r], kind, f"rank {r}")
            assert (got[nb:] == SENT).all(), f"rank {r} guard"
            outs.append([got])
        for side, bufs, i, keepl in (("send", sends, 0, so),
                                     ("recv", recvs, 1, ro)):
            got = bufs[r].cpu().numpy()
            nb = sizes[r][i]
            assert nb == ref[side][r].nbytes, (r, side)
            same(got[:nb], ref[side][r], kind, f"rank {r} {side} staging")
            # nothing beyond the (kept) bytes is ever written
            assert (got[nb:] == SENT).all(), f"rank {r} {side} guard"
            keepl.append(got)
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)
    return outs, so, ro


def assert_same_bytes(a, b):
    """Two ``run_hop`` results, byte for byte, guards included."""
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            if isinstance(u, list):
                for s, t in zip(u, v):
                    assert s.tobytes() == t.tobytes()
            else:
                assert u.tobytes() == v.tobytes()
