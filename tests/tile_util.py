"""Helpers for the device tests of the 4-/8-/16-byte tiles
(test_gpu_word_tiles.py): bit-pattern buffers of any power-of-two element
size, a pa_device_copy runner, and the whole-buffer sentinel compare.

Host buffers are numpy arrays of an unsigned integer type (``uint8`` ..
``uint64``; two ``uint64`` fields for 16-byte elements), so the CPU executor
``apply_copy`` indexes them in element units.  Device buffers are ``uint8``
tensors: slicing one by ``k * esz`` bytes moves the base pointer by ``k``
elements without involving a torch dtype of that width.
"""

from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from pencilarrays_amd import native
from pencilarrays_amd.copyexec import apply_copy
from pencilarrays_amd.plan import CopyDesc

I64 = ctypes.c_int64
SENTINEL = 0xAB

NP_BITS = {
    1: np.dtype(np.uint8), 2: np.dtype(np.uint16), 4: np.dtype(np.uint32),
    8: np.dtype(np.uint64),
    16: np.dtype([("lo", np.uint64), ("hi", np.uint64)]),
}


def rand_bits(rng, n: int, esz: int) -> np.ndarray:
    """``n`` elements of ``esz`` random bytes each."""
    return rng.integers(0, 256, n * esz, dtype=np.uint8).view(NP_BITS[esz])


def sentinel_np(n: int, esz: int) -> np.ndarray:
    a = np.empty(n, dtype=NP_BITS[esz])
    a.view(np.uint8)[:] = SENTINEL
    return a


def same_bytes(a: np.ndarray, b: np.ndarray) -> bool:
    a = np.ascontiguousarray(a).view(np.uint8)
    b = np.ascontiguousarray(b).view(np.uint8)
    return a.shape == b.shape and np.array_equal(a, b)


def to_gpu(a: np.ndarray, slice_elems: int = 0):
    """Upload the bytes of ``a`` behind ``slice_elems`` elements of padding;
    the returned tensor starts at the data, so its base pointer sits
    ``slice_elems`` elements into the allocation."""
    esz = a.dtype.itemsize
    raw = np.ascontiguousarray(a).view(np.uint8)
    if slice_elems:
        raw = np.concatenate(
            [np.full(slice_elems * esz, 0x5C, dtype=np.uint8), raw])
    return torch.from_numpy(raw).to("cuda:0")[slice_elems * esz:]


def sentinel_gpu(n: int, esz: int, slice_elems: int = 0):
    t = torch.full(((n + slice_elems) * esz,), SENTINEL, dtype=torch.uint8,
                   device="cuda:0")
    return t[slice_elems * esz:]


def to_np(t, esz: int) -> np.ndarray:
    return t.cpu().numpy().view(NP_BITS[esz])


def dev_copy(desc: CopyDesc, esz: int, src_t, dst_t) -> None:
    lib = native.load()
    nd = len(desc.dims)
    st = lib.pa_device_copy(
        nd, (I64 * nd)(*desc.dims), (I64 * nd)(*desc.sstrides),
        I64(desc.soffset), (I64 * nd)(*desc.dstrides), I64(desc.doffset),
        I64(esz), ctypes.c_void_p(src_t.data_ptr()),
        ctypes.c_void_p(dst_t.data_ptr()), None)
    assert st == 0, lib.pa_last_error().decode()


def kernel_of(desc: CopyDesc, esz: int, src_t, dst_t) -> native.KernelKind:
    return native.copy_kernel_kind(desc, esz, src_t.data_ptr(),
                                   dst_t.data_ptr())


def extent(desc: CopyDesc, strides, offset: int) -> int:
    """Elements a buffer needs to hold every index the descriptor touches."""
    return offset + 1 + sum((n - 1) * s for n, s in zip(desc.dims, strides))


def run_desc(desc: CopyDesc, esz: int, src: np.ndarray, dst_n: int,
             src_slice: int = 0, dst_slice: int = 0,
             exp: Optional[np.ndarray] = None,
             want=None) -> native.KernelKind:
    """Run ``desc`` through pa_device_copy from ``src`` into a sentinel-filled
    destination of ``dst_n`` elements and compare the WHOLE destination bit
    for bit with ``exp`` (default: the CPU executor on a sentinel-filled
    buffer).  ``*_slice`` moves that base pointer by so many elements.
    ``want`` = (kind, word_bytes, sweep_depth) is asserted BEFORE the copy
    runs.  Returns the selection."""
    assert extent(desc, desc.sstrides, desc.soffset) <= src.size
    assert extent(desc, desc.dstrides, desc.doffset) <= dst_n
    if exp is None:
        exp = sentinel_np(dst_n, esz)
        apply_copy(desc, src, exp)
    assert exp.size == dst_n
    src_t = to_gpu(src, src_slice)
    dst_t = sentinel_gpu(dst_n, esz, dst_slice)
    k = kernel_of(desc, esz, src_t, dst_t)
    what = f"esz={esz} {desc} slice=({src_slice},{dst_slice}) kind={k}"
    assert k.byteified == 0, what
    if want is not None:
        assert (k.kind, k.word_bytes, k.sweep_depth) == tuple(want), what
    dev_copy(desc, esz, src_t, dst_t)
    torch.cuda.synchronize()
    assert same_bytes(to_np(dst_t, esz), exp), what
    return k


def transpose_desc(n0, nta, nb, s_pitch, soff, d_pitch, doff,
                   s_batch=None, d_batch=None) -> CopyDesc:
    """src axis 0 unit-stride with row pitch ``s_pitch``; dst unit-stride
    along axis 1 with row pitch ``d_pitch``; axis 2 is batch (dense on top
    of the rows unless a batch stride is given)."""
    return CopyDesc(
        dims=(n0, nta, nb),
        sstrides=(1, s_pitch, s_pitch * nta if s_batch is None else s_batch),
        soffset=soff,
        dstrides=(d_pitch, 1, d_pitch * n0 if d_batch is None else d_batch),
        doffset=doff)
