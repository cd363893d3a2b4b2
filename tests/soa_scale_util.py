"""Helpers shared by the scaled split / join transpose tests.

References never come from the code under test: the multiply is numpy on the
real view (``scale_util.ref_scale``), the placement is the C oracle per
component (``soa_util.split_case`` / ``join_case``), applied to the
reference-scaled component copies.  Buffers are compared whole as bit
patterns, NaN for NaN-ness (``wire_util.assert_same`` on the real view)."""

from __future__ import annotations

import math

import numpy as np

from many_util import expected_dests
from scale_util import ALPHAS, F32, F64, assert_same, ref_scale
from soa_util import interleave, join_case, split_case

# kind -> (array dtype, scalar bytes S, real scalar dtype R, PA_SCALAR code)
KINDS = {
    "f32": (np.dtype(np.float32), 4, np.dtype(np.float32), F32),
    "f64": (np.dtype(np.float64), 8, np.dtype(np.float64), F64),
    "c64": (np.dtype(np.complex64), 8, np.dtype(np.float32), F32),
    "c128": (np.dtype(np.complex128), 16, np.dtype(np.float64), F64),
}


def pick_alpha(i: int) -> float:
    """One of the issue's alphas, cycled by a case counter."""
    return ALPHAS[i % len(ALPHAS)]


def scale_bytes(raw: np.ndarray, kind: str, alpha: float) -> np.ndarray:
    """``raw`` (uint8) read as scalars of ``kind``, reference-scaled, as
    bytes again."""
    return ref_scale(raw.view(KINDS[kind][0]), alpha).view(np.uint8)


def same(got, exp, kind: str, what="") -> None:
    """Whole buffers (any dtype of the same bytes) as bit patterns of the
    real scalar, NaN for NaN-ness."""
    R = KINDS[kind][2]
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
    e = np.ascontiguousarray(exp).reshape(-1).view(np.uint8)
    assert g.size == e.size, (what, g.size, e.size)
    assert_same(g.view(R), e.view(R), what)


def scaled_split_case(cfg, kind, n, alpha, oracle_lib_path, seed=0x50A1):
    """``(aos, scaled, exp)``: the random source parents ``aos[r]`` (bytes),
    the reference-scaled component copies ``scaled[c][r]`` and the oracle's
    destinations ``exp[c][r]`` of those."""
    ssz = KINDS[kind][1]
    aos, comps, _ = split_case(cfg, ssz, n, oracle_lib_path, seed)
    scaled = [[scale_bytes(x, kind, alpha) for x in row] for row in comps]
    return aos, scaled, expected_dests(scaled, cfg, ssz, oracle_lib_path)


def scaled_join_case(cfg, kind, n, alpha, oracle_lib_path, seed=0x501A):
    """``(fields, scaled, exp_c, exp)``: random scalar source parents
    ``fields[c][r]``, their reference-scaled copies, the oracle's transposes
    ``exp_c[c][r]`` of those and the interleave ``exp[r]``."""
    ssz = KINDS[kind][1]
    fields, _, _ = join_case(cfg, ssz, n, oracle_lib_path, seed)
    scaled = [[scale_bytes(x, kind, alpha) for x in row] for row in fields]
    exp_c = expected_dests(scaled, cfg, ssz, oracle_lib_path)
    nr = math.prod(cfg[1])
    exp = [interleave([exp_c[c][r] for c in range(n)], ssz)
           for r in range(nr)]
    return fields, scaled, exp_c, exp
