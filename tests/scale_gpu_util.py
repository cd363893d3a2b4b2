"""Device-side helpers of the scaled-transpose tests: a pa_device_copy_scale
runner that asserts the selection first and compares the WHOLE sentinel-filled
destination with the numpy reference, and the stage API run as a multi-rank
transpose on one GPU, scaled and unscaled on the same inputs."""

from __future__ import annotations

import math

import numpy as np
import torch

from keep_util import expected_keep
from pencilarrays_amd import build_plan, native
from scale_util import (
    KINDS, SCALE_KINDS, assert_same, expected_rows, expected_scaled,
    kind_parents, pencils, plan_of, plan_rows, ref_scale, seeded_values,
)
from wire_gpu_util import GUARD, SENT, dev, extent, sentinel

CODE = {np.dtype(np.float32): native.SCALAR_F32,
        np.dtype(np.float64): native.SCALAR_F64}


def ref_copy_scale(desc, src, dst, nscal, alpha):
    """The descriptor (element units of ``nscal`` scalars) on the host over
    flat scalar arrays, multiplying with the numpy reference."""
    dims, sstr, soff, dstr, doff = desc
    if 0 in dims:
        return
    isz = src.itemsize
    ast = np.lib.stride_tricks.as_strided
    shape = tuple(dims) + (nscal,)
    sv = ast(src[soff * nscal:], shape=shape,
             strides=tuple(s * nscal * isz for s in sstr) + (isz,))
    dv = ast(dst[doff * nscal:], shape=shape,
             strides=tuple(s * nscal * isz for s in dstr) + (isz,))
    dv[...] = ref_scale(np.ascontiguousarray(sv), alpha)


def run_copy_scale(desc, S, nscal, alpha, seed, want_kind=None, want_vec=None,
                   src_lead=0, dst_lead=0, slack=4, src=None):
    """Run ``desc`` through pa_device_copy_scale.  Buffers are just large
    enough plus ``slack`` scalars and a guard; ``*_lead`` moves that base
    pointer so many SCALARS into its allocation.  The selection is asserted
    with the real pointers before the copy runs; the whole destination (lead,
    data, slack, guard) is compared.  Returns the selection."""
    S = np.dtype(S)
    dims, sstr, soff, dstr, doff = desc
    if src is None:
        src = seeded_values(extent(dims, sstr, soff, nscal) + slack, S, seed)
    assert src.dtype == S
    dst_n = extent(dims, dstr, doff, nscal) + slack
    exp = np.empty(dst_n, dtype=S)
    exp.view(np.uint8)[:] = SENT
    ref_copy_scale(desc, src, exp, nscal, alpha)

    isz = S.itemsize
    s_all = torch.cat([torch.full((src_lead * isz,), 0x5C, dtype=torch.uint8,
                                  device="cuda:0"), dev(src)])
    s_t = s_all[src_lead * isz:]
    d_all = sentinel(dst_lead * isz + dst_n * isz)
    d_t = d_all[dst_lead * isz:]
    k = native.copy_kernel_kind_scale(desc, CODE[S], nscal, s_t.data_ptr(),
                                      d_t.data_ptr())
    what = f"{S} nscal={nscal} a={alpha} {desc} " \
           f"lead=({src_lead},{dst_lead}) {k}"
    if want_kind is not None:
        assert k.kind == want_kind, what
    else:
        assert k.kind in SCALE_KINDS, what
    if want_vec is not None:
        assert k.vec == want_vec, what
    native.device_copy_scale(desc, CODE[S], nscal, alpha, s_t.data_ptr(),
                             d_t.data_ptr())
    torch.cuda.synchronize()
    got = d_all.cpu().numpy()
    lead_b, nb = dst_lead * isz, dst_n * isz
    assert (got[:lead_b] == SENT).all(), what + " lead"
    assert (got[lead_b + nb:] == SENT).all(), what + " guard"
    assert got.size == lead_b + nb + GUARD
    assert_same(got[lead_b:lead_b + nb].view(S), exp, what)
    return k


def expected_of(kind, parents, cfg, alpha, keep, oracle_lib_path):
    """``exp[f][r]`` in the array dtype: the C oracle on the reference-scaled
    input, masked to ``keep`` with the complement zero where given."""
    dtype, elem, S, code, nscal = KINDS[kind]
    if keep is None:
        return expected_scaled(kind, parents, cfg, alpha, oracle_lib_path)
    scaled = [[ref_scale(p, alpha).view(np.uint8) for p in row]
              for row in parents]
    exp = expected_keep(scaled, cfg, np.dtype(S).itemsize * nscal, keep,
                        oracle_lib_path)
    return [[e.view(dtype) for e in row] for row in exp]


def _run(cfg, kind, parents, exp, alpha, aliased, keep, lead, rows_hook):
    """One pass of every rank through pack_many -> slice copies ->
    local_many -> unpack_many, with plans scaled by ``alpha`` (None: without a
    scale; the destinations are then not compared).  Returns the bytes of
    every staging buffer, guards included."""
    dtype, elem, S, code, nscal = KINDS[kind]
    n, nr = len(parents), len(parents[0])
    isz = np.dtype(S).itemsize
    Pi, Po = pencils(cfg)
    pyplans = [build_plan(Pi, Po, r, cfg[6], aliased=aliased, keep=keep)
               for r in range(nr)]
    plans = [plan_of(cfg, r, kind, aliased, keep, alpha=alpha)
             for r in range(nr)]

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

    # launch rows through the queries, real pointers, before anything runs
    if alpha is not None:
        for r, p in enumerate(plans):
            plain = plan_of(cfg, r, kind, aliased, keep)
            plain.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
            want = expected_rows(plain, n, code, nscal, sp[r], dp[r],
                                 recvs[r].data_ptr())
            got = plan_rows(p, n, sp[r], dp[r])
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

    out = {"send": [t.cpu().numpy() for t in sends],
           "recv": [t.cpu().numpy() for t in recvs]}
    for r in range(nr):
        for f in range(n):
            got = d_all[r][f].cpu().numpy()
            lb, nb = lead_b(f), exp[f][r].nbytes
            assert got.size == lb + nb + GUARD
            assert (got[:lb] == SENT).all(), f"rank {r} field {f} lead"
            assert (got[lb + nb:] == SENT).all(), f"rank {r} field {f} guard"
            if alpha is not None:
                assert_same(got[lb:lb + nb].view(dtype), exp[f][r],
                            f"rank {r} field {f}")
        for name, nbytes in (("send", sizes[r][0]), ("recv", sizes[r][1])):
            assert (out[name][r][nbytes:] == SENT).all(), \
                f"rank {r} {name} guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)
    return out


def run_stage_sim_scaled(cfg, kind, n, alpha, oracle_lib_path, aliased=False,
                         keep=None, lead=None, rows_hook=None, seed=0x5CA1):
    """All ranks of ``cfg`` on one GPU through the stage API, once with plans
    without a scale and once with scaled plans on the same inputs.  Asserts
    the scaled plan's rows against ``expected_rows`` (and ``rows_hook(rank,
    rows_by_stage)``), every destination against the C oracle on the scaled
    input, every guard in both runs, and that the two runs leave
    byte-identical staging buffers.  ``lead[f]``: field ``f`` starts that many
    scalars into its allocations."""
    lead = lead or {}
    parents = kind_parents(kind, cfg, n, oracle_lib_path, seed)
    exp = expected_of(kind, parents, cfg, alpha, keep, oracle_lib_path)
    a = _run(cfg, kind, parents, exp, None, aliased, keep, lead, None)
    b = _run(cfg, kind, parents, exp, alpha, aliased, keep, lead, rows_hook)
    for r in range(math.prod(cfg[1])):
        for name in ("send", "recv"):
            assert np.array_equal(a[name][r], b[name][r]), (r, name)
