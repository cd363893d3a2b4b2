"""Helpers shared by the split / join transpose tests.

A vector-valued array is ``n`` scalars of ``ssz`` bytes per element,
components fastest.  References never come from the code under test: a
component is a numpy slice of the array's bytes, and its transpose is the C
oracle's, which moves opaque elements of ``ssz`` bytes.  Everything is
compared as bytes (random bit patterns contain NaNs)."""

from __future__ import annotations

import math

import numpy as np

from many_util import expected_dests, random_parents

# scalar bytes -> the dtype the arrays are typed with
DTYPES = {4: np.float32, 8: np.float64, 16: np.complex128}


def component(aos_bytes: np.ndarray, ssz: int, n: int, c: int) -> np.ndarray:
    """Component ``c`` of an array of ``n``-scalar structs, as bytes."""
    return np.ascontiguousarray(
        aos_bytes.reshape(-1, n, ssz)[:, c, :]).reshape(-1)


def interleave(comps, ssz: int) -> np.ndarray:
    """The array of structs whose component ``c`` is ``comps[c]`` (bytes)."""
    return np.ascontiguousarray(
        np.stack([c.reshape(-1, ssz) for c in comps], axis=1)).reshape(-1)


def elem_type(ssz: int) -> np.dtype:
    """A numpy type of ``ssz`` bytes that assignment moves as opaque bits."""
    return np.dtype({4: np.uint32, 8: np.uint64, 16: np.complex128}[ssz])


def desc_extent(dims, strides, offset: int) -> int:
    """Scalars a field needs to hold every index one side of a descriptor
    touches (the vector-valued side needs ``n`` times as many)."""
    return offset + 1 + sum((d - 1) * s for d, s in zip(dims, strides))


def ref_copy_soa(desc, aos_u8, fields_u8, ssz: int, n: int, split: bool):
    """One split / join copy on ``uint8`` host buffers by plain index
    arithmetic: ``desc`` = (dims, sstr, soff, dstr, doff) of one component in
    scalars; scalar ``c`` of element ``e`` of the vector-valued side sits at
    ``n*e + c``."""
    dims, sstr, soff, dstr, doff = desc
    grids = np.meshgrid(*[np.arange(d, dtype=np.int64) for d in dims],
                        indexing="ij")
    si = soff + sum(g * s for g, s in zip(grids, sstr))
    di = doff + sum(g * s for g, s in zip(grids, dstr))
    si, di = np.asarray(si).reshape(-1), np.asarray(di).reshape(-1)
    dt = elem_type(ssz)
    A = aos_u8.view(dt)
    for c in range(n):
        F = fields_u8[c].view(dt)
        if split:
            F[di] = A[si * n + c]
        else:
            A[di * n + c] = F[si]


def split_case(cfg, ssz, n, oracle_lib_path, seed=0x50A1):
    """``(aos, comps, exp)`` of a split over ``cfg`` = (dims, pdims, di, pi,
    do, po, extra): ``aos[r]`` the random vector-valued source parent of rank
    ``r`` (bytes), ``comps[c][r]`` its component copies, ``exp[c][r]`` the
    oracle's destination of field ``c``."""
    dims, pdims, di, pi, do, po, extra = cfg
    aos = random_parents(dims, pdims, di, extra, ssz * n, 1, oracle_lib_path,
                         seed)[0]
    comps = [[component(a, ssz, n, c) for a in aos] for c in range(n)]
    return aos, comps, expected_dests(comps, cfg, ssz, oracle_lib_path)


def join_case(cfg, ssz, n, oracle_lib_path, seed=0x501A):
    """``(fields, exp_c, exp)`` of a join: ``fields[c][r]`` random scalar
    source parents (bytes), ``exp_c[c][r]`` the oracle's transpose of each,
    ``exp[r]`` their interleave: the vector-valued destination parent."""
    dims, pdims, di, pi, do, po, extra = cfg
    fields = random_parents(dims, pdims, di, extra, ssz, n, oracle_lib_path,
                            seed)
    exp_c = expected_dests(fields, cfg, ssz, oracle_lib_path)
    nr = math.prod(pdims)
    exp = [interleave([exp_c[c][r] for c in range(n)], ssz)
           for r in range(nr)]
    return fields, exp_c, exp
