"""Helpers shared by the elem_dims tests (vector-valued elements, components
fastest): seeded inputs with interleaved parents, and the C oracle run at
``esz = ncomp * itemsize``."""

from __future__ import annotations

import math

import numpy as np

import oracle as orc
from util import COracle


def seeded_elem_parents(dims, pdims, decomp, perm, extra, dtype, elem_dims,
                        seed=0xE1E7):
    """(global array of shape elem_dims + dims + extra, per-rank interleaved
    parent flats of scalars).  Values are random bit patterns of ``dtype``'s
    width, so every byte of an element is distinguishable."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    shape = tuple(elem_dims) + tuple(dims) + tuple(extra)
    g = rng.integers(0, 256, size=math.prod(shape) * dt.itemsize,
                     dtype=np.uint8).view(dt).reshape(shape)
    ncomp = math.prod(elem_dims)
    # component index c = e0 + E0*e1 + ... (axis 0 fastest)
    gc = g.reshape((ncomp,) + tuple(dims) + tuple(extra), order="F")
    parents = []
    for r in range(math.prod(pdims)):
        comps = [orc.parent_from_global(gc[c], dims, pdims, decomp, perm, r,
                                        extra) for c in range(ncomp)]
        parents.append(np.ascontiguousarray(
            np.stack(comps, axis=0).ravel(order="F")))
    return g, parents


def c_oracle_elem(oracle_lib_path, parents, dims, pdims, di, pi, do, po,
                  extra, dtype, ncomp):
    """Expected dest parents (flats of scalars) from the C oracle moving
    opaque elements of ``ncomp * itemsize`` bytes."""
    dt = np.dtype(dtype)
    outs = COracle(oracle_lib_path).transpose_all(
        parents, dims, pdims, di, pi, do, po, extra, dt.itemsize * ncomp)
    return [o.view(dt) for o in outs]


def same_bits(a, b) -> bool:
    """Bit-for-bit equality (random bit patterns contain NaNs)."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        a.tobytes() == b.tobytes()
