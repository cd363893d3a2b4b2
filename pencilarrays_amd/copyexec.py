"""CPU execution of :class:`CopyDesc` strided copies via numpy.

This is the host-side mirror of the HIP copy engine, used by the CPU
(gloo-tested) path and by unit tests.  The GPU product path never runs this —
it executes the same descriptors with HIP kernels through the C ABI.
"""

from __future__ import annotations

import numpy as np

from .plan import CopyDesc, FillDesc


def apply_copy(desc: CopyDesc, src_flat: np.ndarray, dst_flat: np.ndarray) -> None:
    """dst[doffset + Σ j·dstrides] = src[soffset + Σ j·sstrides]."""
    if desc.nelem == 0:
        return
    assert src_flat.ndim == 1 and dst_flat.ndim == 1
    isz = src_flat.itemsize
    assert dst_flat.itemsize == isz
    sv = np.lib.stride_tricks.as_strided(
        src_flat[desc.soffset:],
        shape=desc.dims,
        strides=tuple(s * isz for s in desc.sstrides),
    )
    dv = np.lib.stride_tricks.as_strided(
        dst_flat[desc.doffset:],
        shape=desc.dims,
        strides=tuple(s * isz for s in desc.dstrides),
    )
    dv[...] = sv


def apply_copy_conv(desc: CopyDesc, src_scalars: np.ndarray,
                    dst_scalars: np.ndarray, ncomp: int, conv) -> None:
    """The converting copy of a reduced-precision wire plan: ``desc`` in
    ELEMENT units over flat SCALAR arrays of ``ncomp`` scalars per element
    (components fastest), which may differ in dtype;
    ``dst = conv(src)`` elementwise (wire.narrow / wire.widen / their
    composition)."""
    if desc.nelem == 0:
        return
    assert src_scalars.ndim == 1 and dst_scalars.ndim == 1
    si, di = src_scalars.itemsize, dst_scalars.itemsize
    sv = np.lib.stride_tricks.as_strided(
        src_scalars[desc.soffset * ncomp:],
        shape=tuple(desc.dims) + (ncomp,),
        strides=tuple(s * ncomp * si for s in desc.sstrides) + (si,),
    )
    dv = np.lib.stride_tricks.as_strided(
        dst_scalars[desc.doffset * ncomp:],
        shape=tuple(desc.dims) + (ncomp,),
        strides=tuple(s * ncomp * di for s in desc.dstrides) + (di,),
    )
    dv[...] = conv(sv)


def apply_copy_soa(desc: CopyDesc, aos_scalars: np.ndarray,
                   field: np.ndarray, n: int, c: int, split: bool) -> None:
    """Component ``c`` of a split or join copy: ``desc`` is the descriptor of
    one component in scalar units, and the array of structs holds scalar
    ``c`` of element ``e`` at ``n*e + c``.  ``split``: the source side
    addresses ``aos_scalars`` and the destination side ``field``; otherwise
    the reverse."""
    if desc.nelem == 0:
        return
    assert aos_scalars.ndim == 1 and field.ndim == 1
    isz = field.itemsize
    assert aos_scalars.itemsize == isz
    astr, aoff = (desc.sstrides, desc.soffset) if split else \
        (desc.dstrides, desc.doffset)
    fstr, foff = (desc.dstrides, desc.doffset) if split else \
        (desc.sstrides, desc.soffset)
    av = np.lib.stride_tricks.as_strided(
        aos_scalars[aoff * n + c:], shape=desc.dims,
        strides=tuple(s * n * isz for s in astr))
    fv = np.lib.stride_tricks.as_strided(
        field[foff:], shape=desc.dims, strides=tuple(s * isz for s in fstr))
    if split:
        fv[...] = av
    else:
        av[...] = fv


def apply_fill(desc: FillDesc, dst_flat: np.ndarray) -> None:
    """dst[doffset + Σ j·dstrides] = +0 (all zero bytes): the fill of a
    truncated transpose outside its keep set."""
    if desc.nelem == 0:
        return
    assert dst_flat.ndim == 1
    isz = dst_flat.itemsize
    dv = np.lib.stride_tricks.as_strided(
        dst_flat[desc.doffset:],
        shape=desc.dims,
        strides=tuple(s * isz for s in desc.dstrides),
    )
    dv[...] = np.zeros((), dtype=dst_flat.dtype)
