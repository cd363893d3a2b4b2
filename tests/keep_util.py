"""Helpers shared by the truncated-transpose tests.  No expected value here
uses the plan code under test: the keep set becomes a numpy boolean mask over
the global index space, ownership comes from the oracle's ``owned_region``,
and the expected destinations are the C oracle run on the masked input.  The
expected launch rows at the end restate the grouping rules over the Python
plan's descriptors and the per-descriptor host queries."""

from __future__ import annotations

import math

import numpy as np

import oracle as orc
from many_util import _oracle, ceil_div, expected_workgroups
from pencilarrays_amd import native
from pencilarrays_amd.plan import stage_descs

ID3 = (0, 1, 2)
ID4 = (0, 1, 2, 3)

# (dims, pdims, decomp_in, perm_in, decomp_out, perm_out, extra)
CFG_22 = ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ())
CFG_14 = ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ())
CFG_SLAB = ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ())
CFG_EMPTY = ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ())
CFG_4D = ((6, 7, 8, 9), (2, 2), (1, 3), ID4, (0, 3), (3, 0, 1, 2), ())  # SWEEP[18]
CFG_EXTRA = ((8, 9, 10), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), (3,))
CPU_CFGS = [CFG_22, CFG_14, CFG_SLAB, CFG_EMPTY, CFG_4D, CFG_EXTRA]


def cfg_id(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}_e{c[6]}"


def full_keep(dims):
    return [(N, 0) for N in dims]


def hop_dims(cfg):
    """(u, v, P): the logical dim decomposed along the changing topology
    dimension before (u) and after (v) the transpose, and its process count."""
    _, pdims, di, _, do, _, _ = cfg
    j = next(j for j in range(len(pdims)) if di[j] != do[j])
    return di[j], do[j], pdims[j]


def keep_sets(cfg):
    """The named keep sets of the issue for ``cfg``, cut relative to the
    rank boundaries ``N*c//P`` of the dim ``v`` that the destination splits."""
    dims = cfg[0]
    u, v, P = hop_dims(cfg)
    Nu, Nv = dims[u], dims[v]
    b1 = Nv // P            # first rank boundary along v
    blast = Nv * (P - 1) // P

    def ks(**by_dim):
        k = full_keep(dims)
        for d, ab in by_dim.items():
            k[int(d[1:])] = ab
        return k

    out = {
        "inside": ks(**{f"d{v}": (b1 + 1, 0)}),
        "boundary": ks(**{f"d{v}": (b1, 0)}),
        "droprank": ks(**{f"d{v}": (blast, 0)}),
        "two_dims": ks(**{f"d{v}": (b1 + 1, 0),
                          f"d{u}": (-(-2 * Nu // 3), 0)}),
        "nothing": ks(**{f"d{u}": (0, 0)}),
        "full": ks(**{"d0": (dims[0] - 1, 1)}),
    }
    # b > 0 with both ranges inside one block: a dim that neither pencil
    # splits, else a gap inside the first rank's share of v
    free = [d for d in range(len(dims)) if d not in cfg[2] and d not in cfg[4]]
    if free:
        out["two_ranges"] = ks(**{f"d{free[0]}": (2, 3)})
    else:
        assert b1 >= 3, cfg
        out["two_ranges"] = ks(**{f"d{v}": (1, Nv - (b1 - 1))})
    return out


KEEP_NAMES = ["inside", "boundary", "droprank", "two_ranges", "two_dims",
              "nothing", "full"]


def keep_mask(dims, keep):
    """Boolean mask of the keep set over the global index space."""
    m = np.ones(dims, dtype=bool)
    for d, (ab, N) in enumerate(zip(keep, dims)):
        a, b = (N, 0) if ab is None else ab
        kd = np.zeros(N, dtype=bool)
        kd[:a] = True
        kd[N - b:] = True
        shape = [1] * len(dims)
        shape[d] = N
        m &= kd.reshape(shape)
    return m


def owner_mask(dims, pdims, decomp, rank):
    m = np.zeros(dims, dtype=bool)
    m[tuple(slice(lo, hi) for lo, hi in
            orc.owned_region(dims, pdims, decomp, rank))] = True
    return m


def pair_counts(cfg, keep):
    """``c[r][q]`` = |rank r's source box ∩ rank q's destination box ∩ K|,
    in global indices (extra dims not counted)."""
    dims, pdims, di, _, do, _, _ = cfg
    nr = math.prod(pdims)
    K = keep_mask(dims, keep)
    src = [owner_mask(dims, pdims, di, r) for r in range(nr)]
    dst = [owner_mask(dims, pdims, do, r) for r in range(nr)]
    return [[int((src[r] & dst[q] & K).sum()) for q in range(nr)]
            for r in range(nr)]


def parent_mask(cfg, keep, rank, side):
    """The keep mask in the layout of ``rank``'s parent (one bool per
    element); ``side`` 0 = input pencil, 1 = output pencil."""
    dims, pdims, di, pi, do, po, extra = cfg
    K = keep_mask(dims, keep)
    full = np.broadcast_to(K.reshape(K.shape + (1,) * len(extra)),
                           tuple(dims) + tuple(extra))
    dec, perm = (di, pi) if side == 0 else (do, po)
    return orc.parent_from_global(full, dims, pdims, dec, perm, rank, extra)


def expected_keep(parents, cfg, esz, keep, oracle_lib_path, fill_zero=True,
                  sentinel=0xAB):
    """``exp[f][r]`` (uint8): the C oracle on the numpy-masked input.  With
    ``fill_zero=False`` the complement holds ``sentinel`` bytes instead."""
    dims, pdims, di, pi, do, po, extra = cfg
    nr = math.prod(pdims)
    lib = _oracle(oracle_lib_path)
    smask = [parent_mask(cfg, keep, r, 0) for r in range(nr)]
    dmask = [parent_mask(cfg, keep, r, 1) for r in range(nr)]
    out = []
    for f in range(len(parents)):
        masked = []
        for r in range(nr):
            p = parents[f][r].reshape(-1, esz).copy()
            p[~smask[r]] = 0
            masked.append(p.reshape(-1))
        exp = lib.transpose_all(masked, dims, pdims, di, pi, do, po, extra,
                                esz)
        if not fill_zero:
            for r in range(nr):
                e = exp[r].reshape(-1, esz)
                e[~dmask[r]] = sentinel
        out.append(exp)
    return out


# ---- expected launch rows of ordinary and keep plans (host queries) -----

def _tup(d):
    return (d.dims, d.sstrides, d.soffset, d.dstrides, d.doffset)


def _wg(desc, kk, ssz, ncomp):
    """Workgroups by the documented grid rules, None where the kind has
    none restated in the tests."""
    if kk.byteified:
        return None
    if kk.kind == native.KERNEL_GENERIC:
        return min(ceil_div(math.prod(desc[0]), 256), 8192)
    if kk.kind in (native.KERNEL_COPY_1D, native.KERNEL_LINEAR,
                   native.KERNEL_TILE, native.KERNEL_TILE_VS,
                   native.KERNEL_TILE_PK, native.KERNEL_TILE_WIDE):
        return expected_workgroups(desc, kk, ssz, ncomp)
    return None


def expected_rows(pl, n, stage, ssz, ncomp, sp, dp, send, recv):
    """The rows pa_plan_stage_launches must report, from the Python plan's
    sub-box tables and the per-descriptor queries with the real pointers:
    linear-family entries of one word share a grouped row, TILE / TILE_VS at
    sweep 1 likewise, anything else is a row of its own; the fill entries of
    every field share ONE grouped row at the end of the local stage.
    ``workgroups`` is None where it is not checked."""
    rows = []   # [kind, grouped, entries, workgroups, word]

    def add(kind, grouped, wg, word):
        if grouped:
            for r in rows:
                if r[1] and r[0] == kind and r[4] == word:
                    r[2] += 1
                    r[3] = None if wg is None or r[3] is None else r[3] + wg
                    return
        rows.append([kind, grouped, 1, wg, word])

    for f in range(n):
        for which, d in stage_descs(pl, n, f, stage):
            src = sp[f] if which in (0, 1, 3) else recv
            dst = {1: send, 3: recv}.get(which, dp[f] if dp else 0)
            kk = native.copy_kernel_kind(d, ssz, src, dst, ncomp)
            wg = _wg(_tup(d), kk, ssz, ncomp)
            if kk.kind in (native.KERNEL_COPY_1D, native.KERNEL_LINEAR):
                add(native.KERNEL_LINEAR, True, wg, kk.word_bytes)
            elif kk.kind in (native.KERNEL_TILE, native.KERNEL_TILE_VS) \
                    and kk.sweep_depth == 1:
                add(kk.kind, True, wg, kk.word_bytes)
            else:
                add(kk.kind, False, wg, kk.word_bytes)
    if stage == native.STAGE_LOCAL:
        for f in range(n):
            for fd in pl.fills:
                fk = native.fill_kernel_kind(fd, ssz, dp[f], ncomp)
                assert fk.kind == native.KERNEL_FILL
                lanes = (fd.nelem * ssz * ncomp // fk.store_bytes
                         if fd.dstrides[0] == 1 else fd.nelem)
                add(native.KERNEL_FILL, True, ceil_div(lanes, 256), 0)
    return rows


def check_rows(p, pl, n, ssz, ncomp, sp, dp, send, recv):
    for stage in (native.STAGE_PACK, native.STAGE_LOCAL, native.STAGE_UNPACK):
        got = p.stage_launches(n, stage, sp, dp)
        want = expected_rows(pl, n, stage, ssz, ncomp, sp, dp, send, recv)
        assert [(l.kind, l.grouped, l.entries) for l in got] == \
            [(w[0], w[1], w[2]) for w in want], (stage, got, want)
        for l, w in zip(got, want):
            if w[3] is not None:
                assert l.workgroups == w[3], (stage, l, w)
    return p.stage_launches(n, native.STAGE_LOCAL, sp, dp)
