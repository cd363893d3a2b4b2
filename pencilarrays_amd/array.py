"""PencilArray: local array + decomposition metadata.

Mirrors the slice of src/arrays.jl the hot path and its parity checks need:

- the parent (local storage) has the dimensions of the pencil in **memory**
  order plus optional extra dims appended on the slowest side
  (arrays.jl:134-138); memory axis 0 is the fastest-varying, so the flat
  buffer is byte-identical to the reference's column-major Julia parent.
- logical-order accessors ``size_local`` / ``range_local`` (size.jl,
  arrays.jl:317-340 index-permutation semantics).

Storage backends:
- numpy ndarray (host mirror, used by CPU/gloo tests and the oracle recipes);
- torch tensor on ROCm (``cuda``) — the product path, whose data movement is
  done exclusively by the native HIP engine.

The parent is held as a FLAT 1-D buffer plus (mem_dims,) metadata; views in
memory or logical order are materialised on demand.  This avoids committing to
either C or Fortran axis conventions in the storage itself.

Vector-valued elements (``elem_dims``): an element may be a small array of
``prod(elem_dims)`` scalars of the storage dtype with the COMPONENTS FASTEST
(array of structs) — the reference's ``PencilArray{SVector{3,Float64}}``,
which it moves as one 24-byte element.  The flat buffer then holds
``ncomp * prod(mem_dims)`` scalars; ``mem_dims``, ``len()`` and every plan
quantity keep counting elements.  ``extra_dims`` is the other layout: the
components on the slowest axes (structure of arrays).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from .pencil import Pencil
from .permutations import perm_inv


class PencilArray:
    def __init__(self, pencil: Pencil, rank: int, data_flat,
                 extra_dims: Tuple[int, ...] = (),
                 elem_dims: Tuple[int, ...] = ()):
        self.pencil = pencil
        self.rank = rank
        self.extra_dims = tuple(int(e) for e in extra_dims)
        self.elem_dims = tuple(int(c) for c in elem_dims)
        if any(c < 1 for c in self.elem_dims):
            raise ValueError(f"elem_dims must be positive: {self.elem_dims}")
        self.ncomp = math.prod(self.elem_dims)  # scalars per element
        mem = tuple(pencil.size_local(rank, memory_order=True)) + self.extra_dims
        self.mem_dims = mem
        want = self.ncomp * math.prod(mem)
        if data_flat.ndim != 1 or data_flat.shape[0] != want:
            raise ValueError(
                f"array has incorrect dimensions: {data_flat.shape}. "
                f"Expected flat length {want} for memory dims {mem}"
                + (f" of elements {self.elem_dims}." if self.elem_dims
                   else "."))
        self.data = data_flat  # flat, length ncomp * prod(mem_dims)

    # ---- constructors --------------------------------------------------

    @classmethod
    def empty(cls, pencil: Pencil, rank: int, dtype="float64",
              extra_dims: Tuple[int, ...] = (), backend: Optional[str] = None,
              device=None, elem_dims: Tuple[int, ...] = ()):
        if backend is None:  # a device implies torch storage
            backend = "numpy" if device is None else "torch"
        mem = tuple(pencil.size_local(rank, memory_order=True)) + tuple(extra_dims)
        n = math.prod(mem) * math.prod(tuple(elem_dims))
        if backend == "numpy":
            flat = np.empty(n, dtype=dtype)
        elif backend == "torch":
            import torch
            flat = torch.empty(n, dtype=getattr(torch, str(dtype)) if isinstance(dtype, str) else dtype,
                               device=device)
        else:
            raise ValueError(backend)
        return cls(pencil, rank, flat, extra_dims, elem_dims)

    # ---- views ---------------------------------------------------------

    @property
    def is_torch(self) -> bool:
        return not isinstance(self.data, np.ndarray)

    def parent_memview(self):
        """Parent array with axes in memory order, axis 0 fastest.

        numpy: a Fortran-ordered view of shape ``mem_dims``.
        torch: a view of shape ``reversed(mem_dims)`` permuted so that the
        returned tensor has shape ``mem_dims`` with axis 0 fastest.
        With ``elem_dims`` the shape is ``elem_dims + mem_dims`` (the
        components are the fastest axes).
        """
        shape = self.elem_dims + self.mem_dims
        if self.is_torch:
            t = self.data.view(tuple(reversed(shape)))
            nd = len(shape)
            return t.permute(tuple(range(nd - 1, -1, -1)))
        return self.data.reshape(shape, order="F")

    def element_view(self):
        """numpy only: the flat buffer as ``prod(mem_dims)`` opaque elements
        of ``ncomp * itemsize`` bytes — what the copy descriptors (element
        units) index.  The flat itself when there are no ``elem_dims``."""
        if not self.elem_dims:
            return self.data
        return self.data.view(
            np.dtype((np.void, self.ncomp * self.data.itemsize)))

    def logical_view(self):
        """Local array with axes in LOGICAL order (+ extra axes): index
        [i0,...,iN-1] like the reference's ``u[i,j,k]`` (arrays.jl:327-337).
        With ``elem_dims`` the shape is ``elem_dims + logical + extra``."""
        n = self.pencil.ndims
        e = len(self.extra_dims)
        c = len(self.elem_dims)
        mv = self.parent_memview()
        # mem axis i holds logical dim perm[i]; logical dim d is mem axis
        # inv(perm)[d].
        invp = perm_inv(self.pencil.perm)
        order = tuple(range(c)) + tuple(c + i for i in invp) + \
            tuple(range(c + n, c + n + e))
        if self.is_torch:
            return mv.permute(order)
        return mv.transpose(order)

    def size_local(self, memory_order: bool = False) -> Tuple[int, ...]:
        s = self.pencil.size_local(self.rank, memory_order)
        return tuple(s) + self.extra_dims

    def similar(self, pencil: Optional[Pencil] = None, dtype=None) -> "PencilArray":
        """similar(x, [p::Pencil]) (arrays.jl:287-303): a new uninitialised
        PencilArray with the same (or the given) decomposition, same backend
        and device."""
        p = self.pencil if pencil is None else pencil
        if self.is_torch:
            import torch
            dt = self.data.dtype if dtype is None else dtype
            return PencilArray.empty(p, self.rank, dtype=dt,
                                     extra_dims=self.extra_dims,
                                     backend="torch",
                                     device=self.data.device,
                                     elem_dims=self.elem_dims)
        dt = self.data.dtype if dtype is None else dtype
        return PencilArray.empty(p, self.rank, dtype=dt,
                                 extra_dims=self.extra_dims,
                                 elem_dims=self.elem_dims)

    def __len__(self):
        return int(math.prod(self.mem_dims))
