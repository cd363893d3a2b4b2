"""gather: collect the full (global, logical-order) array — the parity oracle
recipe used by every reference transpose test (src/gather.jl, used by
test/transpose.jl:6-22).

Two forms:
- :func:`gather_sim` — in-process: takes all ranks' PencilArrays, returns the
  global array.  Mirrors gather.jl:59-95 placement: dest[axes_all[n]] = block.
- :func:`gather_dist` — torch.distributed form (gloo/nccl): non-root ranks
  inverse-permute their parent (gather.jl:32-40) and send (:49-56); root
  receives per-rank blocks and places them (:68-95).  Returns the array on
  root, None elsewhere.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .array import PencilArray
from .dtypes import bits_dtype, to_numpy

MPI_TAG = 42  # gather.jl:23


def _logical_block(x: PencilArray) -> np.ndarray:
    """Local data as a contiguous array in logical order (+ extra dims) —
    the inverse-permuted copy of gather.jl:32-40."""
    lv = x.logical_view()
    if x.is_torch:
        lv = to_numpy(lv)
    return np.ascontiguousarray(lv)


def gather_sim(arrays: Sequence[PencilArray]) -> np.ndarray:
    """Global logical-order array from all ranks' PencilArrays, of shape
    ``elem_dims + size_global + extra_dims``.  Torch data
    of a dtype numpy cannot represent (``torch.bfloat16``) comes back as the
    same-width unsigned-integer bit pattern (``uint16``), placed exactly as
    ``int16`` data would be."""
    p0 = arrays[0].pencil
    extra = arrays[0].extra_dims
    elem = arrays[0].elem_dims
    shape = elem + tuple(p0.size_global) + extra
    first = arrays[0].data
    dtype = first.dtype if isinstance(first, np.ndarray) else \
        bits_dtype(first.dtype)
    dest = np.empty(shape, dtype=dtype)
    for r, x in enumerate(arrays):
        assert x.rank == r
        region = x.pencil.axes_for_rank(r)
        sl = tuple(slice(None) for _ in elem) + \
            tuple(slice(lo, hi) for lo, hi in region) + \
            tuple(slice(None) for _ in extra)
        dest[sl] = _logical_block(x)
    return dest


def gather_dist(x: PencilArray, root: int = 0) -> Optional[np.ndarray]:
    """Distributed gather to ``root`` (None elsewhere).  As in
    :func:`gather_sim`, torch dtypes without a numpy counterpart
    (``torch.bfloat16``) are gathered as ``uint16`` bit patterns."""
    import torch
    import torch.distributed as dist

    comm_rank = dist.get_rank()
    block = _logical_block(x)
    out_dtype = block.dtype
    if out_dtype == np.uint16 and x.is_torch:
        block = block.view(np.int16)  # bit patterns travel as int16

    if comm_rank != root:
        dist.send(torch.from_numpy(block), dst=root, tag=MPI_TAG)
        return None

    p = x.pencil
    extra = x.extra_dims
    elem = x.elem_dims
    shape = elem + tuple(p.size_global) + extra
    dest = np.empty(shape, dtype=out_dtype)
    topo = p.topology
    for r in range(topo.nranks):
        region = p.axes_for_rank(r)
        sl = tuple(slice(None) for _ in elem) + \
            tuple(slice(lo, hi) for lo, hi in region) + \
            tuple(slice(None) for _ in extra)
        if r == root:
            dest[sl] = block.view(out_dtype)
        else:
            dims = elem + tuple(hi - lo for lo, hi in region) + extra
            buf = torch.empty(dims, dtype=torch.from_numpy(block).dtype)
            dist.recv(buf, src=r, tag=MPI_TAG)
            dest[sl] = buf.numpy().view(out_dtype)
    return dest
