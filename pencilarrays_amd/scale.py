"""Scaled transposes: ``dest = alpha * T(src)``, the normalisation of an
inverse FFT folded into the pass that writes the destination
(include/pencilhip.h, pa_plan_set_scale), and the numpy multiply of the host
mirror.

The contract's multiply is ONE IEEE multiply per real scalar of type ``S``
(float32 or float64) by ``a = S(alpha)``: round to nearest even, subnormals
kept.  A complex item is two scalars scaled one by one, so the host mirror
multiplies on the real view; numpy's complex * real differs on inf and NaN.
"""

from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

# scalar codes of include/pencilhip.h
SCALAR_F32 = 1
SCALAR_F64 = 2

_REAL_OF = {"float64": ("float64", 1), "float32": ("float32", 1),
            "complex128": ("float64", 2), "complex64": ("float32", 2)}


class Scale(NamedTuple):
    code: int         # SCALAR_F32 / SCALAR_F64
    real: np.dtype    # the real scalar type S of the arrays
    comps: int        # scalars per array item (2 for complex)
    alpha: float      # as given; the kernels multiply by S(alpha)

    @property
    def a(self):
        """``S(alpha)``: alpha rounded to nearest even to the scalar type."""
        with np.errstate(over="ignore", under="ignore"):
            return self.real.type(self.alpha)


def resolve_scale(dtype, scale) -> Optional[Scale]:
    """The scale of a transpose of arrays of ``dtype`` (numpy or torch dtype,
    or its name) by ``scale``; ``None`` for ``scale`` ``None`` or ``1.0``,
    which mean "no scale".  ``ValueError`` for a dtype other than float32,
    float64, complex64 or complex128 and for a NaN or infinite value."""
    if scale is None:
        return None
    name = str(dtype)
    if name.startswith("torch."):
        name = name[len("torch."):]
    else:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            pass
    if name not in _REAL_OF:
        raise ValueError(
            f"scale needs arrays of float32, float64, complex64 or "
            f"complex128, not {name}")
    alpha = float(scale)
    if not math.isfinite(alpha):
        raise ValueError(f"scale must be finite, got {scale!r}")
    if alpha == 1.0:
        return None
    real, comps = _REAL_OF[name]
    return Scale(SCALAR_F32 if real == "float32" else SCALAR_F64,
                 np.dtype(real), comps, alpha)


def scale_array(array: np.ndarray, scale) -> np.ndarray:
    """The contract's ``src (*) a`` on a numpy array: every real scalar (the
    real and imaginary parts of a complex item) times ``S(scale)``.  Returns
    a new array of the input's dtype and shape."""
    x = np.ascontiguousarray(array)
    s = resolve_scale(x.dtype, scale)
    if s is None:
        return x.copy()
    with np.errstate(all="ignore"):
        out = x.view(s.real) * s.a
    return out.view(x.dtype).reshape(x.shape)
