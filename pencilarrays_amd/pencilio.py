"""Parallel binary I/O in the reference's MPIIODriver on-disk format
(src/PencilIO/mpi_io.jl + PencilIO.jl:55-65) — §8(f) row 4.

Format (bit-compatible with the reference, version 0.9.4):

- one raw binary file, datasets appended back to back;
- **discontiguous** (default, chunks=false): a dataset is the GLOBAL array
  stored in MEMORY order (column-major over ``dims_memory`` =
  permutation*global dims + extra dims + collection dims) — what
  ``MPI.Types.create_subarray`` over ``size_global(MemoryOrder())`` produces
  (mpi_io.jl:364-380).  Readable with any process count/decomposition.
- **contiguous** (chunks=true): per-process parent blocks, ordered by the
  COLUMN-MAJOR linear index of the process in the topology
  (``LinearIndices(topo)[coords]``, mpi_io.jl:406-418) — readable only with
  the same topology (:326-333).
- ``<file>.json`` metadata written by rank 0 (mpi_io.jl:99-110): driver
  {type, version}, datasets {name: {permutation (1-based, null if identity),
  extra_dims, decomposed_dims (1-based), process_dims, julia_endian_bom,
  little_endian, element_type (Julia name), dims_logical, dims_memory,
  chunks, offset_bytes, size_bytes}} (:194-211).

Transport here is plain POSIX I/O through numpy memmaps (single node — the
page cache makes concurrent per-rank window writes coherent); an MPI host
would use MPI-IO with the identical layout.  Synchronisation uses
torch.distributed barriers when initialised.
"""

from __future__ import annotations

import json
import math
import os
import sys
from typing import Tuple

import numpy as np

from .array import PencilArray
from .dtypes import numpy_dtype
from .permutations import is_identity, perm_apply

MPIIO_VERSION = "0.9.4"

_JULIA_TYPES = {
    "float64": "Float64", "float32": "Float32", "float16": "Float16",
    "complex64": "ComplexF32", "complex128": "ComplexF64",
    "int64": "Int64", "int32": "Int32", "int16": "Int16", "int8": "Int8",
    "uint64": "UInt64", "uint32": "UInt32", "uint16": "UInt16",
    "uint8": "UInt8", "bool": "Bool",
}
_NUMPY_TYPES = {v: k for k, v in _JULIA_TYPES.items()}


def _unsupported(name: str) -> TypeError:
    return TypeError(
        f"MPIIODriver: unsupported element type {name} (supported: "
        f"{sorted(_JULIA_TYPES)})")


def _reject_elem_dims(x) -> None:
    """The on-disk metadata describes scalar element types only: it has no
    place for vector-valued elements, so such arrays are refused."""
    if getattr(x, "elem_dims", ()):
        raise NotImplementedError(
            f"pencilio does not support arrays with elem_dims "
            f"(got elem_dims={x.elem_dims}): the file metadata cannot "
            f"describe vector-valued elements")


def _julia_type(dtype: np.dtype) -> str:
    try:
        return _JULIA_TYPES[dtype.name]
    except KeyError:
        raise _unsupported(dtype.name) from None


def _data_dtype(data) -> np.dtype:
    """numpy element type of a PencilArray's data (numpy or torch); torch
    dtypes numpy cannot represent (bfloat16) are unsupported on disk."""
    if isinstance(data, np.ndarray):
        return data.dtype
    dt = numpy_dtype(data.dtype)
    if dt is None:
        raise _unsupported(str(data.dtype).replace("torch.", ""))
    return dt


def _barrier():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
    except ImportError:
        pass


def _colmajor_rank_order(topo):
    """Process order of the chunked layout: column-major linear index over
    Cartesian coords (LinearIndices(topo), mpi_io.jl:406-418)."""
    order = []
    dims = topo.dims
    n = topo.nranks
    for lin in range(n):
        coords = []
        rem = lin
        for d in dims:  # first topology dim fastest (Julia column-major)
            coords.append(rem % d)
            rem //= d
        order.append(topo.cart_rank(tuple(coords)))
    return order


class MPIIOFile:
    """open(MPIIODriver(), filename, comm) (mpi_io.jl:140-145).

    mode "w" truncates and writes metadata on close; "r" expects the JSON
    metadata next to the file (or reads dataset 0 blindly via read_raw)."""

    def __init__(self, filename: str, mode: str = "r", rank: int = 0):
        self.filename = filename
        self.mode = mode
        self.rank = rank
        self.position = 0
        if mode == "w":
            self.meta = {
                "driver": {"type": "MPIIODriver", "version": MPIIO_VERSION},
                "datasets": {},
            }
            if rank == 0:
                open(filename, "wb").close()
            _barrier()
        else:
            metafile = filename + ".json"
            if os.path.exists(metafile):
                with open(metafile) as fh:
                    self.meta = json.load(fh)
            else:
                self.meta = {"datasets": {}}

    # ---- write -------------------------------------------------------

    def write(self, name: str, x: PencilArray, chunks: bool = False):
        """setindex!(file, x, name; chunks) (mpi_io.jl:172-189)."""
        _reject_elem_dims(x)
        p = x.pencil
        offset = self.position
        dtype = _data_dtype(x.data)
        _julia_type(dtype)  # unsupported types fail before touching the file
        esz = x.data.dtype.itemsize if isinstance(x.data, np.ndarray) else \
            x.data.element_size()
        size_bytes = (math.prod(p.size_global)
                      * math.prod(x.extra_dims or (1,)) * esz)

        if self.rank == 0:
            with open(self.filename, "r+b") as fh:
                fh.truncate(offset + size_bytes)
        _barrier()

        local = x.data if isinstance(x.data, np.ndarray) else \
            x.data.cpu().numpy()
        n = p.ndims
        e = len(x.extra_dims)

        if chunks:
            my_off = offset + self._chunk_offset(x, esz)
            with open(self.filename, "r+b") as fh:
                fh.seek(my_off)
                fh.write(local.tobytes())
        else:
            dims_mem = tuple(perm_apply(p.perm, p.size_global)) + x.extra_dims
            mm = np.memmap(self.filename, dtype=dtype, mode="r+",
                           offset=offset, shape=dims_mem, order="F")
            window = tuple(
                slice(lo, hi)
                for lo, hi in p.range_local(self.rank, memory_order=True)
            ) + tuple(slice(None) for _ in x.extra_dims)
            mm[window] = local.reshape(x.mem_dims, order="F")
            mm.flush()
            del mm
        _barrier()

        # Identity => null: the reference's Tuple(NoPermutation()) is
        # `nothing` (its own test uses `perm === nothing`, test/io.jl:60-63)
        # and JSON3 writes nothing as null — byte-faithful.
        perm_json = (None if is_identity(p.perm)
                     else [v + 1 for v in p.perm])
        self.meta["datasets"][name] = {
            "permutation": perm_json,
            "extra_dims": list(x.extra_dims),
            "decomposed_dims": [d + 1 for d in p.decomp_dims],
            "process_dims": list(p.topology.dims),
            "julia_endian_bom": "0x04030201" if sys.byteorder == "little"
            else "0x01020304",
            "little_endian": sys.byteorder == "little",
            "element_type": _julia_type(dtype),
            "dims_logical": list(p.size_global) + list(x.extra_dims),
            "dims_memory": list(dims_mem_of(p, x.extra_dims)),
            "chunks": chunks,
            "offset_bytes": offset,
            "size_bytes": size_bytes,
        }
        self.position = offset + size_bytes

    def _chunk_offset(self, x: PencilArray, esz: int) -> int:
        p = x.pencil
        pex = math.prod(x.extra_dims or (1,))
        order = _colmajor_rank_order(p.topology)
        my_lin = order.index(self.rank)
        off = 0
        for lin in range(my_lin):
            off += p.length_local(order[lin]) * pex
        return off * esz

    # ---- read --------------------------------------------------------

    def read(self, name: str, x: PencilArray):
        """read!(file, x, name) (mpi_io.jl:232-263): checks element type,
        memory dims, byte size and endianness (check_metadata :293-325)."""
        _reject_elem_dims(x)
        meta = self.meta["datasets"].get(name)
        if meta is None:
            raise KeyError(f"dataset '{name}' not found")
        p = x.pencil
        dtype = _data_dtype(x.data)
        if meta["element_type"] != _julia_type(dtype):
            raise TypeError(
                f"incompatible type of file and array: "
                f"{meta['element_type']} != {_julia_type(dtype)}")
        dims_mem = dims_mem_of(p, x.extra_dims)
        if tuple(meta["dims_memory"]) != tuple(dims_mem):
            raise ValueError(
                f"incompatible dimensions of dataset in file and array: "
                f"{meta['dims_memory']} != {dims_mem}")
        # size_bytes consistency (check_metadata's @assert, mpi_io.jl:306-307)
        want_bytes = (math.prod(p.size_global)
                      * math.prod(x.extra_dims or (1,)) * dtype.itemsize)
        if "size_bytes" in meta and meta["size_bytes"] != want_bytes:
            raise ValueError(
                f"dataset '{name}' size_bytes {meta['size_bytes']} != "
                f"computed global size {want_bytes}")
        want_bom = "0x04030201" if sys.byteorder == "little" else "0x01020304"
        if meta.get("julia_endian_bom", want_bom) != want_bom:
            raise ValueError("file endianness does not match this system")
        if meta["chunks"]:
            if tuple(meta["process_dims"]) != tuple(p.topology.dims):
                raise ValueError(
                    f"dataset '{name}' was written in chunks with a "
                    f"different topology ({meta['process_dims']} != "
                    f"{p.topology.dims})")
        self._read_at(x, meta["offset_bytes"], meta["chunks"], np.dtype(dtype))
        return x

    def read_raw(self, x: PencilArray, offset: int = 0):
        """read!(file, x; offset) without metadata (mpi_io.jl:265-278)."""
        _reject_elem_dims(x)
        dtype = _data_dtype(x.data)
        self._read_at(x, offset, False, np.dtype(dtype))
        return x

    def _read_at(self, x: PencilArray, offset: int, chunks: bool, dtype):
        p = x.pencil
        if chunks:
            my_off = offset + self._chunk_offset(x, dtype.itemsize)
            n = math.prod(x.mem_dims)
            with open(self.filename, "rb") as fh:
                fh.seek(my_off)
                buf = np.frombuffer(fh.read(n * dtype.itemsize), dtype=dtype)
        else:
            dims_mem = tuple(perm_apply(p.perm, p.size_global)) + x.extra_dims
            mm = np.memmap(self.filename, dtype=dtype, mode="r",
                           offset=offset, shape=dims_mem, order="F")
            window = tuple(
                slice(lo, hi)
                for lo, hi in p.range_local(self.rank, memory_order=True)
            ) + tuple(slice(None) for _ in x.extra_dims)
            buf = np.asfortranarray(mm[window]).ravel(order="F")
            del mm
        if isinstance(x.data, np.ndarray):
            x.data[:] = buf
        else:
            import torch
            x.data.copy_(torch.from_numpy(buf.copy()).to(x.data.device))

    # ---- close -------------------------------------------------------

    def close(self):
        if self.mode == "w" and self.rank == 0:
            with open(self.filename + ".json", "w") as fh:
                json.dump(self.meta, fh, indent=4)
                fh.write("\n")
        _barrier()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def dims_mem_of(p, extra_dims) -> Tuple[int, ...]:
    return tuple(perm_apply(p.perm, p.size_global)) + tuple(extra_dims)
