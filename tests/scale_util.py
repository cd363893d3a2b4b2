"""Helpers shared by the scaled-transpose tests.

The reference that defines "exact" is numpy on the REAL view of an array,
``x.view(S) * S(alpha)`` -- one IEEE multiply per real scalar, round to
nearest even, subnormals kept -- never the code under test, and never numpy's
complex * real, which differs on inf and NaN.  Results are compared as bit
patterns, NaN for NaN-ness only (wire_util.assert_same).  Expected launch rows
never come from the scaled plan: the UNSCALED plan's descriptors, the
selection query per descriptor and the grid rules below give them."""

from __future__ import annotations

import math

import numpy as np

from pencilarrays_amd import Pencil, Topology, native
from wire_util import assert_same, oracle  # noqa: F401  (re-exported)

F32, F64 = native.SCALAR_F32, native.SCALAR_F64
LIN, TILE, GEN = (native.KERNEL_SCALE_LINEAR, native.KERNEL_SCALE_TILE,
                  native.KERNEL_SCALE_GENERIC)
SCALE_KINDS = {LIN, TILE, GEN}
STAGES = (native.STAGE_PACK, native.STAGE_LOCAL, native.STAGE_UNPACK)
A = 256  # the address the engine assumes for a pointer it is not given

# the alphas of the issue; 1e-320 is a float64 subnormal and 0 in float32
ALPHAS = [0.5, 1.0 / 3.0, -2.0, 1.0 / (130 * 67 * 35), 0.0, 1e-320]

# element kinds: id -> (array dtype, elem_dims, real scalar dtype, code,
# real scalars per element)
KINDS = {
    "f32": (np.float32, (), np.float32, F32, 1),
    "f64": (np.float64, (), np.float64, F64, 1),
    "c64": (np.complex64, (), np.float32, F32, 2),
    "c128": (np.complex128, (), np.float64, F64, 2),
    "3xf64": (np.float64, (3,), np.float64, F64, 3),
    "3xf32": (np.float32, (3,), np.float32, F32, 3),
}
CODE = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}


def real_dtype(dtype) -> np.dtype:
    dt = np.dtype(dtype)
    return np.dtype({"c": {8: np.float32, 16: np.float64}.get(dt.itemsize),
                     "f": dt}[dt.kind])


def ref_scale(x: np.ndarray, alpha: float) -> np.ndarray:
    """The contract's ``x (*) S(alpha)``: numpy on the real view."""
    a = np.ascontiguousarray(x)
    S = real_dtype(a.dtype)
    with np.errstate(all="ignore"):
        out = a.view(S).reshape(-1) * S.type(alpha)
    assert out.dtype == S
    return out.view(a.dtype).reshape(a.shape)


def specials(S) -> np.ndarray:
    """+-0, +-inf, NaN, the largest finite value (x 2 -> inf), the smallest
    normal (x 0.5 -> subnormal), odd subnormals (x 0.5: ties to even), and
    values whose third is inexact."""
    S = np.dtype(S)
    fi = np.finfo(S)
    U = {4: np.uint32, 8: np.uint64}[S.itemsize]
    sub = np.array([1, 3, 5, 7, 0x7FF, (1 << (fi.nmant)) - 1],
                   dtype=U).view(S)  # odd subnormal patterns
    with np.errstate(all="ignore"):
        base = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max,
                         fi.tiny, -fi.tiny, fi.tiny * 1.5, 1.0, 3.0, 10.0,
                         -7.0, 1.0 + fi.eps, fi.max / 3], dtype=S)
    return np.concatenate([base, sub, -sub])


def seeded_values(n: int, S, seed: int) -> np.ndarray:
    """``n`` scalars of type ``S``: finite seeded values over many
    magnitudes with the special values at every 5th slot from 2, as far as
    they fit."""
    S = np.dtype(S)
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 5, n)).astype(S)
    sp = specials(S)
    pos = 2 + 5 * np.arange(len(sp))
    keep = pos < n
    x[pos[keep]] = sp[keep]
    return x


def seeded_patterns(n: int, S, seed: int) -> np.ndarray:
    """``n`` random bit patterns of type ``S`` (NaNs included)."""
    S = np.dtype(S)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n * S.itemsize, dtype=np.uint8).view(S)


def pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po))


def plan_of(cfg, r, kind, aliased=False, keep=None, fill=native.FILL_ZERO,
            alpha=None):
    """The native plan of ``cfg`` on rank ``r`` for elements of ``kind``,
    scaled by ``alpha`` where given."""
    dtype, elem, S, code, nscal = KINDS[kind]
    Pi, Po = pencils(cfg)
    p = native.NativePlan(Pi, Po, r, np.dtype(dtype).itemsize, cfg[6],
                          aliased=aliased, ncomp=math.prod(elem), keep=keep,
                          fill=fill)
    if alpha is not None:
        p.set_scale(code, alpha)
    return p


def kind_parents(kind, cfg, n, oracle_lib_path, seed=0x5CA1):
    """``parents[f][r]``: the parent of field ``f`` on rank ``r`` in the
    array dtype of ``kind``, special values included."""
    dtype, elem, S, code, nscal = KINDS[kind]
    dims, pdims, di, _, _, _, extra = cfg
    orc = oracle(oracle_lib_path)
    return [[seeded_values(orc.local_len(dims, pdims, di, extra, r) * nscal,
                           S, seed + 131 * f + r).view(dtype)
             for r in range(math.prod(pdims))] for f in range(n)]


def expected_scaled(kind, parents, cfg, alpha, oracle_lib_path):
    """``exp[f][r]``: the C oracle (opaque elements) run on the
    reference-scaled parents, in the array dtype."""
    dtype, elem, S, code, nscal = KINDS[kind]
    dims, pdims, di, pi, do, po, extra = cfg
    orc = oracle(oracle_lib_path)
    esz = np.dtype(S).itemsize * nscal
    return [[o.view(dtype) for o in orc.transpose_all(
        [ref_scale(p, alpha) for p in row], dims, pdims, di, pi, do, po,
        extra, esz)] for row in parents]


# ---- expected launch rows ---------------------------------------------------

def ceil_div(a, b):
    return -(-a // b)


def tile_shape(code, nscal):
    """Rows of 512 bytes along axis 0, 64 elements along ta."""
    return (128 if code == F32 else 64) // nscal, 64


def scale_workgroups(desc, kk, nscal):
    """Workgroups of the single-descriptor scaling launch of ``desc``
    (normalized, element units) with selection ``kk``: 256 accesses of V
    scalars per workgroup (linear), one workgroup per tile and batch (tile),
    256 scalars per workgroup up to 8192 workgroups (generic)."""
    dims, sstr, _, dstr, _ = desc
    total = math.prod(dims)
    if kk.kind == LIN:
        return ceil_div(total * nscal // kk.vec, 256)
    if kk.kind == GEN:
        return min(ceil_div(total * nscal, 256), 8192)
    assert kk.kind == TILE and sstr[0] == 1
    ta = next(a for a in range(1, len(dims)) if dstr[a] == 1)
    batch = total // (dims[0] * dims[ta])
    return ceil_div(dims[0], kk.tile_i) * ceil_div(dims[ta], kk.tile_j) * batch


def dest_descs(plain, n, f, stage):
    """``(which, descriptor)`` of every destination-side copy field ``f`` of
    ``n`` makes in ``stage`` (local or unpack), in launch order, from the
    UNSCALED native plan ``plain`` (ordinary or keep)."""
    keep = plain.keep is not None
    if stage == native.STAGE_LOCAL:
        blocks = [(0, 0), (4, 0)]
    else:
        blocks = [(2, k) for k in range(plain.nproc_sub)] \
            if plain.r_dim >= 0 else []
    out = []
    for which, k in blocks:
        if keep:
            for s in range(plain.nsub(which, k)):
                out.append((which, plain.copydesc_sub(n, f, which, k, s)))
        else:
            d = plain.copydesc_many(n, f, which, k)
            if d is not None:
                out.append((which, d))
    return out


def partition(per_desc):
    """``[(kind, V, workgroups)]`` in launch order -> the rows of a scaled
    plan: linear entries of one V share a grouped row, so do all tile
    entries, in first-appearance order; generic entries stay alone."""
    rows = []
    for kind, vec, wg in per_desc:
        sig = {LIN: (LIN, vec), TILE: (TILE,)}.get(kind)
        hit = next((r for r in rows if sig is not None and r[0] == sig), None)
        if hit is not None:
            hit[2] += 1
            hit[3] += wg
        else:
            rows.append([sig, kind, 1, wg])
    return [native.StageLaunch(kind, sig is not None, ne, wg)
            for sig, kind, ne, wg in rows]


def expected_rows(plain, n, code, nscal, sp=None, dp=None, recv=A):
    """Per stage, the rows the scaled plan must report: the pack rows of the
    unscaled plan ``plain``; the partition of the per-descriptor selections
    for local and unpack; the unscaled plan's fill row behind the local
    copies."""
    sp = sp or [A] * n
    dp = dp or [A] * n
    out = {native.STAGE_PACK: plain.stage_launches(n, native.STAGE_PACK, sp,
                                                   dp)}
    for stage in (native.STAGE_LOCAL, native.STAGE_UNPACK):
        per = []
        for f in range(n):
            for which, d in dest_descs(plain, n, f, stage):
                src = sp[f] if which == 0 else recv
                kk = native.copy_kernel_kind_scale(d, code, nscal, src, dp[f])
                if kk.kind != native.KERNEL_NONE:
                    per.append((kk.kind, kk.vec,
                                scale_workgroups(d, kk, nscal)))
        rows = partition(per)
        if stage == native.STAGE_LOCAL:
            rows += [l for l in plain.stage_launches(n, stage, sp, dp)
                     if l.kind == native.KERNEL_FILL]
        out[stage] = rows
    return out


def plan_rows(plan, n, sp=None, dp=None):
    return {s: plan.stage_launches(n, s, sp, dp) for s in STAGES}
