"""Helpers shared by the multi-field transpose tests: per-rank parents of
random bytes for ``n`` fields and their expected destinations from the C
oracle, which moves opaque elements of ``esz`` bytes.  Everything is compared
as bytes (random bit patterns contain NaNs)."""

from __future__ import annotations

import math

import numpy as np

from util import COracle

_ORACLES = {}


def _oracle(path):
    if path not in _ORACLES:
        _ORACLES[path] = COracle(path)
    return _ORACLES[path]


def random_parents(dims, pdims, decomp, extra, esz, n, oracle_lib_path,
                   seed=0x3A17):
    """``parents[f][r]``: uint8 parent of field ``f`` on rank ``r``.  A
    transpose is pure data movement, so any bytes serve as a rank's parent."""
    orc = _oracle(oracle_lib_path)
    rng = np.random.default_rng(seed)
    nr = math.prod(pdims)
    return [[rng.integers(0, 256, orc.local_len(dims, pdims, decomp, extra, r)
                          * esz, dtype=np.uint8) for r in range(nr)]
            for _ in range(n)]


def expected_dests(parents, cfg, esz, oracle_lib_path):
    """``exp[f][r]``: uint8 destination parents from the C oracle, per
    field.  ``cfg`` = (dims, pdims, di, pi, do, po, extra)."""
    dims, pdims, di, pi, do, po, extra = cfg
    orc = _oracle(oracle_lib_path)
    return [orc.transpose_all(parents[f], dims, pdims, di, pi, do, po, extra,
                              esz) for f in range(len(parents))]


def ceil_div(a, b):
    return -(-a // b)


def expected_workgroups(desc, kk, esz, ncomp=1):
    """Workgroups of the single-descriptor launch of ``desc`` (the
    ``(dims, sstr, soff, dstr, doff)`` tuple, element units) given its
    kernel selection ``kk`` (native.KernelKind): the grid rules documented in
    DESIGN.md — 256 words per workgroup for the linear family, one workgroup
    per tile (times the sweep depth) for the tile kernels."""
    from pencilarrays_amd import native as nat
    dims, sstr, _, dstr, _ = desc
    total = math.prod(dims)
    B = esz * ncomp
    if kk.kind in (nat.KERNEL_COPY_1D, nat.KERNEL_LINEAR):
        return ceil_div(total * B // kk.word_bytes, 256)
    ta = next(a for a in range(1, len(dims)) if dstr[a] == 1)
    assert sstr[0] == 1
    if kk.kind == nat.KERNEL_TILE_VS:
        ti, tj = 64, 128
    elif kk.kind == nat.KERNEL_TILE:
        ti, tj = (32, 32) if kk.word_bytes == 16 else (128, 64)
    elif kk.kind == nat.KERNEL_TILE_PK:
        ti, tj = 128, 128
    elif kk.kind == nat.KERNEL_TILE_WIDE:
        ti, tj = 256, 16
        while ti > 16 and ti * B > 1536:
            ti //= 2
    else:
        raise AssertionError(kk)
    batch = total // (dims[0] * dims[ta])
    ntj = ceil_div(dims[ta], tj)
    return ceil_div(dims[0], ti) * ceil_div(ntj, kk.sweep_depth) * batch
