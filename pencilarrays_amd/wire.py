"""Reduced-precision wire: the (stored -> wire) scalar pairs of a transpose
whose staging buffers and messages carry a narrower floating-point type than
the arrays (include/pencilhip.h, pa_plan_create_wire), and the numpy
conversions of the host mirror.

``round_wire`` is the contract's ``round_w``: to the wire type with round to
nearest even and back.  Subnormals of the wire type are kept, values beyond
its range become +-inf, +-0 and +-inf are preserved, a NaN stays a NaN.
float32/float16 use ``numpy.astype``; bfloat16 is done on the ``uint32``
pattern (numpy has no such type) and held as ``uint16`` patterns.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

# pair codes of include/pencilhip.h
WIRE_F64_F32 = 1
WIRE_F32_F16 = 2
WIRE_F32_BF16 = 3
# ops of a converting copy
WIRE_NARROW = 0
WIRE_WIDEN = 1
WIRE_ROUND = 2


class WirePair(NamedTuple):
    code: int
    name: str          # canonical wire name: float32 / float16 / bfloat16
    stored: np.dtype   # real scalar type of the arrays
    carrier: np.dtype  # numpy type of one wire scalar (bf16: uint16 patterns)
    comps: int         # stored scalars per array item (2 for complex)


def wire_name(wire_dtype) -> str:
    """``"float32"`` / ``"float16"`` / ``"bfloat16"`` from a name, a numpy
    dtype or a torch dtype."""
    if isinstance(wire_dtype, str):
        name = wire_dtype
    else:
        name = str(wire_dtype)
        if name.startswith("torch."):
            name = name[len("torch."):]
        else:
            try:
                name = np.dtype(wire_dtype).name
            except TypeError:
                pass
    if name not in ("float32", "float16", "bfloat16"):
        raise ValueError(f"unsupported wire dtype {wire_dtype!r}: must be "
                         f"float32, float16 or bfloat16")
    return name


_PAIRS = {
    ("float64", "float32"): (WIRE_F64_F32, np.float32),
    ("float32", "float16"): (WIRE_F32_F16, np.float16),
    ("float32", "bfloat16"): (WIRE_F32_BF16, np.uint16),
}
_REAL_OF = {"float64": ("float64", 1), "float32": ("float32", 1),
            "complex128": ("float64", 2), "complex64": ("float32", 2)}


def resolve_wire(stored_dtype, wire_dtype) -> WirePair:
    """The wire pair for arrays of ``stored_dtype`` (numpy or torch dtype, or
    its name) sent as ``wire_dtype``; ``ValueError`` for any combination the
    engine has no pair for (integers, float64 -> float16, a wire type no
    narrower than the stored one)."""
    wname = wire_name(wire_dtype)
    sname = str(stored_dtype)
    if sname.startswith("torch."):
        sname = sname[len("torch."):]
    else:
        try:
            sname = np.dtype(stored_dtype).name
        except TypeError:
            pass
    if sname not in _REAL_OF:
        raise ValueError(f"no reduced-precision wire for arrays of {sname}")
    real, comps = _REAL_OF[sname]
    if (real, wname) not in _PAIRS:
        raise ValueError(
            f"no wire pair {real} -> {wname}: supported are float64 -> "
            f"float32, float32 -> float16 and float32 -> bfloat16")
    code, carrier = _PAIRS[(real, wname)]
    return WirePair(code, wname, np.dtype(real), np.dtype(carrier), comps)


def narrow(x: np.ndarray, pair: WirePair) -> np.ndarray:
    """Stored scalars -> wire scalars (``pair.carrier``), elementwise."""
    assert x.dtype == pair.stored, (x.dtype, pair.stored)
    if pair.code != WIRE_F32_BF16:
        with np.errstate(over="ignore", invalid="ignore"):
            return x.astype(pair.carrier)
    u = np.ascontiguousarray(x).view(np.uint32)
    # round to nearest even on the pattern; the carry runs into the exponent
    # and ends at inf.  uint64 keeps the sum of an all-ones pattern exact.
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16) \
        .astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    if nan.any():
        r = np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)
    return r


def widen(w: np.ndarray, pair: WirePair) -> np.ndarray:
    """Wire scalars -> stored scalars (exact), elementwise."""
    assert w.dtype == pair.carrier, (w.dtype, pair.carrier)
    if pair.code != WIRE_F32_BF16:
        return w.astype(pair.stored)
    return (np.ascontiguousarray(w).astype(np.uint32) << 16).view(np.float32)


def round_wire(array: np.ndarray, wire_dtype) -> np.ndarray:
    """``round_w`` of the contract on a numpy array: every scalar (the real
    and imaginary parts of a complex item) converted to ``wire_dtype`` and
    back.  Returns a new array of the input's dtype and shape."""
    a = np.ascontiguousarray(array)
    pair = resolve_wire(a.dtype, wire_dtype)
    out = widen(narrow(a.view(pair.stored), pair), pair)
    return out.view(a.dtype).reshape(a.shape)
