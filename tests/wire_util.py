"""Helpers shared by the reduced-precision wire tests.

The references that define "exact": ``numpy.astype`` for float64->float32
and float32->float16, torch on the CPU for float32->bfloat16 — never the
code under test.  Inputs are seeded finite values with the special values of
each pair (ties, subnormal results, overflow to inf, +-0, +-inf and one NaN)
mixed in at fixed positions; results are compared as bit patterns, NaN for
NaN-ness only."""

from __future__ import annotations

import math

import numpy as np
import torch

from util import COracle

# name -> (stored real dtype, wire name, pair code, wire scalar bytes)
PAIRS = {
    "f64_f32": (np.float64, "float32", 1, 4),
    "f32_f16": (np.float32, "float16", 2, 2),
    "f32_bf16": (np.float32, "bfloat16", 3, 2),
}
NARROW, WIDEN, ROUND = 0, 1, 2

# element kinds of the plan-level tests:
# id -> (array dtype, elem_dims, pair name, stored scalars per element)
ELEM_KINDS = {
    "f64": (np.float64, (), "f64_f32", 1),
    "c128": (np.complex128, (), "f64_f32", 2),
    "3xf64": (np.float64, (3,), "f64_f32", 3),
    "f32_f16": (np.float32, (), "f32_f16", 1),
    "f32_bf16": (np.float32, (), "f32_bf16", 1),
}

FLT_MAX = float(np.finfo(np.float32).max)

_SPECIALS = {
    "f64_f32": [
        0.0, -0.0, np.inf, -np.inf, 3.5e38, -3.5e38, 1e-40, 2.0 ** -149,
        2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -30), 1 + 2.0 ** -24,
        1 + 2.0 ** -24 + 2.0 ** -50, 1 + 3 * 2.0 ** -24,
        FLT_MAX * (1 + 2.0 ** -25), np.nan,
    ],
    "f32_f16": [
        0.0, -0.0, np.inf, -np.inf, 65504.0, 65520.0, 65519.9, -65520.0,
        2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10),
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 6e-8, np.nan,
    ],
    "f32_bf16": [
        0.0, -0.0, np.inf, -np.inf, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
        1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), FLT_MAX, -FLT_MAX,
        2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * (1 + 2.0 ** -10), 1e-40,
        np.nan,
    ],
}


def specials(pair: str) -> np.ndarray:
    """The special values of a pair, in its stored type."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array(_SPECIALS[pair], dtype=PAIRS[pair][0])


def ref_narrow(x: np.ndarray, pair: str) -> np.ndarray:
    """Reference stored -> wire (bfloat16 as uint16 patterns)."""
    stored, wname, _, _ = PAIRS[pair]
    x = np.ascontiguousarray(x)
    assert x.dtype == stored
    if wname == "bfloat16":
        t = torch.from_numpy(x).to(torch.bfloat16)
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(wname)


def ref_widen(w: np.ndarray, pair: str) -> np.ndarray:
    """Reference wire -> stored (exact)."""
    stored, wname, _, _ = PAIRS[pair]
    w = np.ascontiguousarray(w)
    if wname == "bfloat16":
        t = torch.from_numpy(w.view(np.int16)).view(torch.bfloat16)
        return t.to(torch.float32).numpy().copy()
    return w.astype(stored)


def ref_round(x: np.ndarray, pair: str) -> np.ndarray:
    """Reference round_w on real or complex arrays of the stored type."""
    stored = PAIRS[pair][0]
    a = np.ascontiguousarray(x)
    r = ref_widen(ref_narrow(a.view(stored).reshape(-1), pair), pair)
    return r.view(a.dtype).reshape(a.shape)


def carrier(pair: str):
    """numpy type of one wire scalar (bfloat16: uint16 patterns)."""
    return np.dtype({"float32": np.float32, "float16": np.float16,
                     "bfloat16": np.uint16}[PAIRS[pair][1]])


def seeded_values(n: int, pair: str, seed: int) -> np.ndarray:
    """``n`` stored scalars: finite seeded values over many magnitudes, with
    the pair's special values at fixed positions (every 7th slot from 3, as
    far as they fit)."""
    stored = PAIRS[pair][0]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) *
         10.0 ** rng.integers(-6, 5, n)).astype(stored)
    sp = specials(pair)
    pos = 3 + 7 * np.arange(len(sp))
    keep = pos < n
    x[pos[keep]] = sp[keep]
    return x


def seeded_patterns(n: int, pair: str, seed: int) -> np.ndarray:
    """``n`` random bit patterns of the stored type (NaNs included; callers
    mask them)."""
    stored = np.dtype(PAIRS[pair][0])
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n * stored.itemsize,
                        dtype=np.uint8).view(stored)


def uint_view(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def isnan_any(a: np.ndarray) -> np.ndarray:
    """NaN mask of a float array or of uint16 bfloat16 patterns."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return (a & 0x7FFF) > 0x7F80
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    return np.isnan(a)


def assert_same(got: np.ndarray, exp: np.ndarray, what="") -> None:
    """Bit-for-bit equality on every non-NaN scalar of ``exp``; NaN where
    ``exp`` is NaN."""
    got = np.ascontiguousarray(got)
    exp = np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, \
        (what, got.dtype, exp.dtype, got.shape, exp.shape)
    nan = isnan_any(exp).reshape(-1)
    g, e = uint_view(got).reshape(-1), uint_view(exp).reshape(-1)
    bad = np.flatnonzero((g != e) & ~nan)
    assert bad.size == 0, \
        f"{what}: {bad.size} scalars differ, first at {bad[:5]}: " \
        f"{g[bad[:5]]} != {e[bad[:5]]}"
    assert isnan_any(got).reshape(-1)[nan].all(), f"{what}: NaN lost"


_ORACLES = {}


def oracle(path) -> COracle:
    if path not in _ORACLES:
        _ORACLES[path] = COracle(path)
    return _ORACLES[path]


def kind_parents(kind, dims, pdims, decomp, extra, n, oracle_lib_path,
                 seed=0x51DE):
    """``parents[f][r]``: the parent of field ``f`` on rank ``r`` in the
    array dtype of ``kind``.  A transpose moves whole elements, so any values
    serve as a rank's parent."""
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    orc = oracle(oracle_lib_path)
    out = []
    for f in range(n):
        row = []
        for r in range(math.prod(pdims)):
            ln = orc.local_len(dims, pdims, decomp, extra, r)
            row.append(seeded_values(ln * nc, pair, seed + 131 * f + r)
                       .view(dtype))
        out.append(row)
    return out


def expected_rounded(kind, parents, cfg, oracle_lib_path):
    """``exp[f][r]``: the C oracle (opaque elements of the STORED size) run
    on the reference-rounded parents, in the array dtype."""
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    dims, pdims, di, pi, do, po, extra = cfg
    esz = np.dtype(PAIRS[pair][0]).itemsize * nc
    orc = oracle(oracle_lib_path)
    exp = []
    for row in parents:
        rounded = [ref_round(p, pair) for p in row]
        outs = orc.transpose_all(rounded, dims, pdims, di, pi, do, po, extra,
                                 esz)
        exp.append([o.view(dtype) for o in outs])
    return exp
