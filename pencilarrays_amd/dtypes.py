"""torch <-> numpy element-type conversion, in one place (gather, I/O).

numpy has no counterpart for some torch dtypes (``torch.bfloat16``).  Pure
data movement does not need one: such tensors cross to numpy as the
same-width unsigned-integer BIT PATTERN (``uint16`` for bfloat16).
"""

from __future__ import annotations

from typing import Optional

import numpy as np

# same-width integer views for torch dtypes numpy cannot represent:
# element size -> (torch signed dtype name to view as, numpy bit-pattern type)
_BITS = {1: ("int8", np.uint8), 2: ("int16", np.uint16),
         4: ("int32", np.uint32), 8: ("int64", np.uint64)}


def numpy_dtype(torch_dtype) -> Optional[np.dtype]:
    """numpy counterpart of a torch dtype, or None when numpy has none
    (e.g. ``torch.bfloat16``)."""
    try:
        return np.dtype(str(torch_dtype).replace("torch.", ""))
    except TypeError:
        return None


def bits_dtype(torch_dtype) -> np.dtype:
    """The dtype :func:`to_numpy` returns: the numpy counterpart, or the
    same-width unsigned integer when there is none."""
    dt = numpy_dtype(torch_dtype)
    if dt is not None:
        return dt
    import torch
    esz = torch.empty(0, dtype=torch_dtype).element_size()
    if esz not in _BITS:
        raise TypeError(f"no bit-pattern view for {torch_dtype}")
    return np.dtype(_BITS[esz][1])


def to_numpy(t) -> np.ndarray:
    """Host numpy copy/view of a torch tensor.  Dtypes without a numpy
    counterpart come back as same-width unsigned-integer bit patterns (the
    tensor is viewed as the signed integer of its width first; bfloat16 ->
    ``torch.int16`` -> ``uint16``)."""
    import torch
    t = t.cpu()
    if numpy_dtype(t.dtype) is not None:
        return t.numpy()
    esz = t.element_size()
    if esz not in _BITS:
        raise TypeError(f"no bit-pattern view for {t.dtype}")
    tname, npt = _BITS[esz]
    return t.view(getattr(torch, tname)).numpy().view(npt)
