"""ctypes host for the native engine (libpencilhip.so, C ABI in
include/pencilhip.h).

The GPU product path runs EXCLUSIVELY through this module: plan building,
pack/unpack/fused-copy kernels and the RCCL exchange all happen inside the
native library.  If the library is missing on a GPU box this module raises —
there is no eager/PyTorch fallback.

RCCL bootstrap: the 128-byte unique id of each 1-D subgroup communicator is
exchanged through the torch.distributed store (any backend); the library then
calls ncclCommInitRank itself (replacing MPI.Cart_sub,
MPITopologies.jl:244-251).  A Julia/MPI host would broadcast the id over MPI
instead — see INTEGRATION.md.
"""

from __future__ import annotations

import ctypes
import os
from typing import Dict, NamedTuple, Optional, Tuple

I64 = ctypes.c_int64
I32 = ctypes.c_int32
VP = ctypes.c_void_p

_LIB = None


def lib_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "libpencilhip.so")


def load() -> ctypes.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"native engine not built: {path} missing. Run "
            f"`python -c 'import __graft_entry__; __graft_entry__.build()'` "
            f"(hipcc, seconds). The GPU path has no fallback.")
    lib = ctypes.CDLL(path)
    lib.pa_last_error.restype = ctypes.c_char_p
    lib.pa_pencil_length_local.restype = I64
    lib.pa_plan_stage_table_builds.restype = I64
    lib.pa_set_stream_min_bytes.restype = I64
    _LIB = lib
    return lib


def _check(lib, status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what}: {lib.pa_last_error().decode()}")


# kernel kinds reported by pa_copy_kernel_kind (include/pencilhip.h)
KERNEL_NONE = 0
KERNEL_COPY_1D = 1
KERNEL_COPY_1D_NT = 2
KERNEL_LINEAR = 3
KERNEL_TILE = 4
KERNEL_TILE_VS = 5
KERNEL_TILE_PK = 6
KERNEL_GENERIC = 7
KERNEL_TILE_WIDE = 8
# converting kernels of a reduced-precision wire (pa_copy_kernel_kind_wire)
KERNEL_CVT_LINEAR = 9
KERNEL_CVT_TILE = 10
KERNEL_CVT_GENERIC = 11
# grouped zero fill of a truncated transpose (pa_fill_kernel_kind)
KERNEL_FILL = 12
FILL_NONE, FILL_ZERO = 0, 1
# scaling kernels of a scaled transpose (pa_copy_kernel_kind_scale)
KERNEL_SCALE_LINEAR = 13
KERNEL_SCALE_TILE = 14
KERNEL_SCALE_GENERIC = 15
# split / join kernels (pa_copy_kernel_kind_soa) and their directions
KERNEL_SOA_LINEAR = 16
KERNEL_SOA_TILE = 17
KERNEL_SOA_GENERIC = 18
SOA_SPLIT, SOA_JOIN = 0, 1
# real scalar types of a scale (pa_plan_set_scale)
SCALAR_F32, SCALAR_F64 = 1, 2
SCALAR_BYTES = {SCALAR_F32: 4, SCALAR_F64: 8}
KERNEL_NAMES = {
    KERNEL_NONE: "NONE", KERNEL_COPY_1D: "COPY_1D",
    KERNEL_COPY_1D_NT: "COPY_1D_NT", KERNEL_LINEAR: "LINEAR",
    KERNEL_TILE: "TILE", KERNEL_TILE_VS: "TILE_VS",
    KERNEL_TILE_PK: "TILE_PK", KERNEL_GENERIC: "GENERIC",
    KERNEL_TILE_WIDE: "TILE_WIDE", KERNEL_CVT_LINEAR: "CVT_LINEAR",
    KERNEL_CVT_TILE: "CVT_TILE", KERNEL_CVT_GENERIC: "CVT_GENERIC",
    KERNEL_FILL: "FILL", KERNEL_SCALE_LINEAR: "SCALE_LINEAR",
    KERNEL_SCALE_TILE: "SCALE_TILE", KERNEL_SCALE_GENERIC: "SCALE_GENERIC",
    KERNEL_SOA_LINEAR: "SOA_LINEAR", KERNEL_SOA_TILE: "SOA_TILE",
    KERNEL_SOA_GENERIC: "SOA_GENERIC",
}

# wire pairs (stored -> wire) and ops of a converting copy
WIRE_F64_F32, WIRE_F32_F16, WIRE_F32_BF16 = 1, 2, 3
WIRE_NARROW, WIRE_WIDEN, WIRE_ROUND = 0, 1, 2
WIRE_STORED_BYTES = {WIRE_F64_F32: 8, WIRE_F32_F16: 4, WIRE_F32_BF16: 4}
WIRE_BYTES = {WIRE_F64_F32: 4, WIRE_F32_F16: 2, WIRE_F32_BF16: 2}


class WireKernelKind(NamedTuple):
    """pa_copy_kernel_kind_wire: ``vec`` scalars per access (linear),
    ``tile_i`` x ``tile_j`` elements per workgroup (tile)."""
    kind: int
    vec: int
    tile_i: int
    tile_j: int
    sweep_depth: int


class KernelKind(NamedTuple):
    kind: int
    word_bytes: int
    byteified: int
    sweep_depth: int
    words_per_element: int = 1


STAGE_PACK, STAGE_LOCAL, STAGE_UNPACK = 0, 1, 2
# flags of the plan creators
PLAN_ALIASED, PLAN_GROUP_CVT, PLAN_GROUP_SOA = 1, 2, 4


class StageLaunch(NamedTuple):
    """One launch of a multi-field stage (pa_plan_stage_launches)."""
    kind: int
    grouped: bool
    entries: int
    workgroups: int


def _desc_fields(desc):
    if hasattr(desc, "sstrides"):
        return (desc.dims, desc.sstrides, desc.soffset, desc.dstrides,
                desc.doffset)
    return desc


def copy_kernel_kind(desc, esz: int, src_ptr: int = 0,
                     dst_ptr: int = 0, ncomp: int = 1) -> KernelKind:
    """Which kernel ``pa_device_copy`` / a plan launches for ``desc`` with
    ``esz``-byte elements (host-only, no GPU needed).  ``desc`` is a
    ``plan.CopyDesc`` or the ``(dims, sstr, soff, dstr, doff)`` tuple of
    ``NativePlan.copydesc``.  The pointers are used for their alignment
    only and never dereferenced.  With ``ncomp > 1`` an element is ``ncomp``
    scalars of ``esz`` bytes, components fastest (pa_copy_kernel_kind_comp);
    ``words_per_element`` is then the fifth field of that query."""
    lib = load()
    if ncomp != 1:
        dims, sstr, soff, dstr, doff = _desc_fields(desc)
        nd = len(dims)
        out = (I64 * 5)()
        _check(lib, lib.pa_copy_kernel_kind_comp(
            nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
            (I64 * nd)(*dstr), I64(doff), I64(esz), I64(ncomp), VP(src_ptr),
            VP(dst_ptr), out), "pa_copy_kernel_kind_comp")
        return KernelKind(*(int(v) for v in out))
    if hasattr(desc, "sstrides"):
        dims, sstr, soff, dstr, doff = (desc.dims, desc.sstrides,
                                        desc.soffset, desc.dstrides,
                                        desc.doffset)
    else:
        dims, sstr, soff, dstr, doff = desc
    nd = len(dims)
    out = (I64 * 4)()
    _check(lib, lib.pa_copy_kernel_kind(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), I64(esz), VP(src_ptr), VP(dst_ptr),
        out), "pa_copy_kernel_kind")
    return KernelKind(*(int(v) for v in out))


def copy_kernel_stream(desc, esz: int, src_ptr: int = 0,
                       dst_ptr: int = 0) -> int:
    """1 when ``pa_device_copy`` runs ``desc`` on the streaming form of the
    vector-store tile (nontemporal loads and vector stores), else 0
    (pa_copy_kernel_stream; host-only, arguments of
    :func:`copy_kernel_kind`)."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    out = I64()
    _check(lib, lib.pa_copy_kernel_stream(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), I64(esz), VP(src_ptr), VP(dst_ptr),
        ctypes.byref(out)), "pa_copy_kernel_stream")
    return int(out.value)


def set_stream_min_bytes(min_bytes: int) -> int:
    """Set the payload size from which the vector-store tile streams and
    return the previous one (pa_set_stream_min_bytes): 0 = always where
    eligible, negative = never.  Process-wide tuning and testing hook."""
    return int(load().pa_set_stream_min_bytes(I64(min_bytes)))


def device_copy(desc, esz: int, src_ptr: int, dst_ptr: int,
                stream: int = 0, ncomp: int = 1) -> None:
    """Run one strided-copy descriptor on the device (pa_device_copy /
    pa_device_copy_comp): elements of ``ncomp`` scalars of ``esz`` bytes."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    args = (nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
            (I64 * nd)(*dstr), I64(doff), I64(esz))
    tail = (VP(src_ptr), VP(dst_ptr), VP(stream))
    if ncomp == 1:
        _check(lib, lib.pa_device_copy(*args, *tail), "pa_device_copy")
    else:
        _check(lib, lib.pa_device_copy_comp(*args, I64(ncomp), *tail),
               "pa_device_copy_comp")


def copy_kernel_kind_wire(desc, wire: int, op: int, ncomp: int = 1,
                          src_ptr: int = 0,
                          dst_ptr: int = 0) -> WireKernelKind:
    """Which converting kernel ``pa_device_copy_wire`` / a wire plan launches
    for ``desc`` (element units, ``ncomp`` scalars per element); host-only,
    the pointers are used for their alignment only."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    out = (I64 * 5)()
    _check(lib, lib.pa_copy_kernel_kind_wire(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), int(wire), int(op), I64(ncomp),
        VP(src_ptr), VP(dst_ptr), out), "pa_copy_kernel_kind_wire")
    return WireKernelKind(*(int(v) for v in out))


def device_copy_wire(desc, wire: int, op: int, ncomp: int, src_ptr: int,
                     dst_ptr: int, stream: int = 0) -> None:
    """Run one converting strided copy on the device
    (pa_device_copy_wire)."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    _check(lib, lib.pa_device_copy_wire(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), int(wire), int(op), I64(ncomp),
        VP(src_ptr), VP(dst_ptr), VP(stream)), "pa_device_copy_wire")


def copy_kernel_kind_scale(desc, scalar: int, nscal: int = 1,
                           src_ptr: int = 0,
                           dst_ptr: int = 0) -> WireKernelKind:
    """Which scaling kernel ``pa_device_copy_scale`` / a scaled plan launches
    for ``desc`` (element units, ``nscal`` scalars of type ``scalar`` per
    element); host-only, the pointers are used for their alignment only.
    The fields are those of :func:`copy_kernel_kind_wire`."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    out = (I64 * 5)()
    _check(lib, lib.pa_copy_kernel_kind_scale(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), int(scalar), I64(nscal),
        VP(src_ptr), VP(dst_ptr), out), "pa_copy_kernel_kind_scale")
    return WireKernelKind(*(int(v) for v in out))


def device_copy_scale(desc, scalar: int, nscal: int, alpha: float,
                      src_ptr: int, dst_ptr: int, stream: int = 0) -> None:
    """Run one scaling strided copy on the device (pa_device_copy_scale):
    ``dst = src * S(alpha)`` per real scalar."""
    lib = load()
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    _check(lib, lib.pa_device_copy_scale(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), int(scalar), I64(nscal),
        ctypes.c_double(alpha), VP(src_ptr), VP(dst_ptr), VP(stream)),
        "pa_device_copy_scale")


def _soa_args(desc, scalar_size: int, n: int, direction: int, aos_ptr: int,
              field_ptrs):
    dims, sstr, soff, dstr, doff = _desc_fields(desc)
    nd = len(dims)
    if field_ptrs is None:
        fields = None
    else:
        if len(field_ptrs) != n:
            raise ValueError(f"expected {n} field pointers, got "
                             f"{len(field_ptrs)}")
        fields = (VP * n)(*[VP(int(q)) for q in field_ptrs])
    return (nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
            (I64 * nd)(*dstr), I64(doff), I64(scalar_size), int(n),
            int(direction), VP(aos_ptr), fields)


def copy_kernel_kind_soa(desc, scalar_size: int, n: int, direction: int,
                         aos_ptr: int = 0,
                         field_ptrs=None) -> WireKernelKind:
    """Which split / join kernel ``pa_device_copy_soa`` / a split or join
    stage launches for ``desc`` (the descriptor of one component, in scalars
    of ``scalar_size`` bytes) between an array of ``n``-scalar structs and
    ``n`` fields; ``direction`` is SOA_SPLIT or SOA_JOIN.  Host-only; the
    pointers (``field_ptrs`` optional) are used for their alignment only.
    The fields are those of :func:`copy_kernel_kind_wire`."""
    lib = load()
    out = (I64 * 5)()
    _check(lib, lib.pa_copy_kernel_kind_soa(
        *_soa_args(desc, scalar_size, n, direction, aos_ptr, field_ptrs),
        out), "pa_copy_kernel_kind_soa")
    return WireKernelKind(*(int(v) for v in out))


def device_copy_soa(desc, scalar_size: int, n: int, direction: int,
                    aos_ptr: int, field_ptrs, stream: int = 0) -> None:
    """Run one split or join copy on the device (pa_device_copy_soa)."""
    lib = load()
    _check(lib, lib.pa_device_copy_soa(
        *_soa_args(desc, scalar_size, n, direction, aos_ptr, field_ptrs),
        VP(stream)), "pa_device_copy_soa")


def device_copy_soa_scale(desc, scalar_size: int, n: int, direction: int,
                          scalar: int, alpha: float, aos_ptr: int, field_ptrs,
                          stream: int = 0) -> None:
    """Run one scaling split or join copy on the device
    (pa_device_copy_soa_scale): every real scalar of type ``scalar`` times
    ``S(alpha)`` on its way; the kernel is the one
    :func:`copy_kernel_kind_soa` reports for the plain copy."""
    lib = load()
    args = _soa_args(desc, scalar_size, n, direction, aos_ptr, field_ptrs)
    _check(lib, lib.pa_device_copy_soa_scale(
        *args[:-2], int(scalar), ctypes.c_double(alpha), *args[-2:],
        VP(stream)), "pa_device_copy_soa_scale")


class FillKernelKind(NamedTuple):
    """pa_fill_kernel_kind: ``store_bytes`` per store of the zero fill."""
    kind: int
    store_bytes: int


def _fill_fields(desc):
    if hasattr(desc, "dstrides"):
        return desc.dims, desc.dstrides, desc.doffset
    return desc


def fill_kernel_kind(desc, esz: int, dst_ptr: int = 0,
                     ncomp: int = 1) -> FillKernelKind:
    """Which stores ``pa_device_fill_zero`` / a keep plan's fill makes for the
    destination-only window ``desc`` (a ``plan.FillDesc`` or ``(dims, dstr,
    doff)``) of ``ncomp`` scalars of ``esz`` bytes; host-only."""
    lib = load()
    dims, dstr, doff = _fill_fields(desc)
    nd = len(dims)
    out = (I64 * 2)()
    _check(lib, lib.pa_fill_kernel_kind(
        nd, (I64 * nd)(*dims), (I64 * nd)(*dstr), I64(doff), I64(esz),
        I64(ncomp), VP(dst_ptr), out), "pa_fill_kernel_kind")
    return FillKernelKind(int(out[0]), int(out[1]))


def device_fill_zero(desc, esz: int, dst_ptr: int, stream: int = 0,
                     ncomp: int = 1) -> None:
    """Zero one destination-only window on the device
    (pa_device_fill_zero)."""
    lib = load()
    dims, dstr, doff = _fill_fields(desc)
    nd = len(dims)
    _check(lib, lib.pa_device_fill_zero(
        nd, (I64 * nd)(*dims), (I64 * nd)(*dstr), I64(doff), I64(esz),
        I64(ncomp), VP(dst_ptr), VP(stream)), "pa_device_fill_zero")


class NativePlan:
    """pa_plan plus the pa_topology/pa_pencil handles it needs.  Plan
    building is host-only (works without a GPU); execute needs one."""

    def __init__(self, Pi, Po, rank: int, elem_size: int,
                 extra_dims: Tuple[int, ...] = (), aliased: bool = False,
                 ncomp: int = 1, wire: Optional[int] = None,
                 keep=None, fill: int = FILL_ZERO, group_cvt: bool = False,
                 group_soa: bool = False):
        """``ncomp > 1``: elements of ``ncomp`` scalars of ``elem_size``
        bytes, components fastest (pa_plan_create_comp).  ``wire``: a wire
        pair code (WIRE_F64_F32, ...) for a reduced-precision wire plan
        (pa_plan_create_wire); ``elem_size`` is then the stored scalar
        size.  ``keep``: ``(a, b)`` per logical dim for a truncated transpose
        (pa_plan_create_keep) with ``fill`` FILL_ZERO or FILL_NONE.
        ``group_cvt``: set PA_PLAN_GROUP_CVT, which on a wire plan groups the
        converting kernels of a stage and has no effect on any other plan.
        ``group_soa``: set PA_PLAN_GROUP_SOA, which on a scalar plan makes the
        split and join stages grouped launches and lets them run on a keep
        plan, and has no effect on any other plan."""
        if keep is not None and wire is not None:
            raise ValueError(
                "a keep set together with a wire pair is not supported")
        lib = self.lib = load()
        topo = Pi.topology
        # both pa_pencils are built against ONE pa_topology handle, so the
        # engine-side topology check can't see a host-level mismatch —
        # validate here (assert_compatible, Transpositions.jl:184-186)
        if tuple(Po.topology.dims) != tuple(topo.dims):
            raise RuntimeError("pencil topologies must be the same.")
        m = topo.ndims
        self._topo = VP()
        _check(lib, lib.pa_topology_create(
            m, (I64 * m)(*topo.dims), ctypes.byref(self._topo)),
            "pa_topology_create")

        def mk_pencil(p):
            h = VP()
            n = p.ndims
            perm = (I32 * n)(*p.perm)
            _check(lib, lib.pa_pencil_create(
                self._topo, n, (I64 * n)(*p.size_global),
                (I32 * m)(*p.decomp_dims), perm, ctypes.byref(h)),
                "pa_pencil_create")
            return h

        self._pi = mk_pencil(Pi)
        self._po = mk_pencil(Po)
        self._plan = VP()
        e = len(extra_dims)
        self.ncomp = int(ncomp)
        self.wire = wire
        self.keep = None
        flags = (PLAN_ALIASED if aliased else 0) | \
            (PLAN_GROUP_CVT if group_cvt else 0) | \
            (PLAN_GROUP_SOA if group_soa else 0)
        if keep is not None:
            keep = list(keep)
            nk = len(keep)
            if nk != Pi.ndims:
                raise ValueError(
                    f"keep needs one (a, b) per logical dim: got {nk} for "
                    f"{Pi.ndims} dims")
            # None = the full range; the engine validates the values
            self.keep = tuple(
                (int(N), 0) if kd is None else (int(kd[0]), int(kd[1]))
                for kd, N in zip(keep, Pi.size_global))
            _check(lib, lib.pa_plan_create_keep(
                self._pi, self._po, I64(elem_size), I64(self.ncomp), e,
                (I64 * e)(*extra_dims) if e else None, rank,
                flags,
                (I64 * nk)(*[a for a, _ in self.keep]),
                (I64 * nk)(*[b for _, b in self.keep]), int(fill),
                ctypes.byref(self._plan)), "pa_plan_create_keep")
        elif wire is None:
            _check(lib, lib.pa_plan_create_comp(
                self._pi, self._po, I64(elem_size), I64(self.ncomp), e,
                (I64 * e)(*extra_dims) if e else None, rank,
                flags,
                ctypes.byref(self._plan)), "pa_plan_create_comp")
        else:
            if WIRE_STORED_BYTES.get(wire, elem_size) != elem_size:
                raise ValueError(
                    f"wire pair {wire} stores {WIRE_STORED_BYTES[wire]}-byte "
                    f"scalars, not {elem_size}")
            _check(lib, lib.pa_plan_create_wire(
                self._pi, self._po, int(wire), I64(self.ncomp), e,
                (I64 * e)(*extra_dims) if e else None, rank,
                flags,
                ctypes.byref(self._plan)), "pa_plan_create_wire")
        self.nproc_sub = lib.pa_plan_nproc_sub(self._plan)
        self.r_dim = lib.pa_plan_r_dim(self._plan)
        self.my_k = lib.pa_plan_my_k(self._plan)

    def plan_wire(self) -> int:
        """The plan's wire pair code, 0 for an ordinary plan
        (pa_plan_wire)."""
        return int(self.lib.pa_plan_wire(self._plan))

    def group_cvt(self) -> bool:
        """True on a wire plan created with ``group_cvt=True``
        (pa_plan_group_cvt)."""
        return bool(self.lib.pa_plan_group_cvt(self._plan))

    def group_soa(self) -> bool:
        """True on a plan created with ``group_soa=True`` on which the flag
        has an effect (pa_plan_group_soa)."""
        return bool(self.lib.pa_plan_group_soa(self._plan))

    def set_scale(self, scalar: int, alpha: float):
        """Make this a scaled plan, ``dest = alpha * T(src)`` per real scalar
        of type ``scalar`` (SCALAR_F32 / SCALAR_F64); ``alpha == 1.0`` takes
        the scale off again (pa_plan_set_scale)."""
        _check(self.lib, self.lib.pa_plan_set_scale(
            self._plan, int(scalar), ctypes.c_double(alpha)),
            "pa_plan_set_scale")

    def plan_scale(self):
        """``(scalar, alpha)`` of a scaled plan (pa_plan_scale), else
        None."""
        sc, al = ctypes.c_int(), ctypes.c_double()
        if not self.lib.pa_plan_scale(self._plan, ctypes.byref(sc),
                                      ctypes.byref(al)):
            return None
        return int(sc.value), float(al.value)

    def buffer_sizes(self) -> Tuple[int, int]:
        s, r = I64(), I64()
        _check(self.lib, self.lib.pa_plan_buffer_sizes(
            self._plan, ctypes.byref(s), ctypes.byref(r)),
            "pa_plan_buffer_sizes")
        return s.value, r.value

    def set_buffers(self, send_ptr: int, recv_ptr: int):
        _check(self.lib, self.lib.pa_plan_set_buffers(
            self._plan, VP(send_ptr), VP(recv_ptr)), "pa_plan_set_buffers")

    def set_comm(self, comm: "NativeComm"):
        _check(self.lib, self.lib.pa_plan_set_comm(self._plan, comm.handle),
               "pa_plan_set_comm")

    def execute(self, src_ptr: int, dst_ptr: int, stream: int):
        _check(self.lib, self.lib.pa_transpose_execute(
            self._plan, VP(src_ptr), VP(dst_ptr), VP(stream)),
            "pa_transpose_execute")

    def wait(self, stream: int):
        _check(self.lib, self.lib.pa_transpose_wait(self._plan, VP(stream)),
               "pa_transpose_wait")

    def enable_timing(self, enable: bool = True):
        """Per-stage HIP-event timing (the TimerOutputs analogue,
        Transpositions.jl:173-177)."""
        _check(self.lib, self.lib.pa_plan_enable_timing(
            self._plan, 1 if enable else 0), "pa_plan_enable_timing")

    def stage_times(self) -> dict:
        """{pack, local, exchange, unpack} in ms for the LAST completed
        execute (call after wait()); absent stages are None."""
        out = (ctypes.c_double * 4)()
        _check(self.lib, self.lib.pa_plan_stage_times(self._plan, out),
               "pa_plan_stage_times")
        keys = ("pack", "local", "exchange", "unpack")
        return {k: (None if out[i] < 0 else out[i])
                for i, k in enumerate(keys)}

    # ---- introspection (host-side; parity tests vs plan.py) ----------

    def block_info(self, k: int):
        out = (I64 * 8)()
        _check(self.lib, self.lib.pa_plan_block_info(self._plan, k, out),
               "pa_plan_block_info")
        return tuple(out)

    def copydesc(self, which: int, k: int = 0):
        nd = I64()
        dims = (I64 * 8)()
        sstr = (I64 * 8)()
        dstr = (I64 * 8)()
        soff = I64()
        doff = I64()
        st = self.lib.pa_plan_copydesc(
            self._plan, which, k, ctypes.byref(nd), dims, sstr,
            ctypes.byref(soff), dstr, ctypes.byref(doff))
        if st != 0:
            return None
        n = nd.value
        return (tuple(dims[:n]), tuple(sstr[:n]), soff.value,
                tuple(dstr[:n]), doff.value)

    # ---- truncated transposes (keep plans) ---------------------------

    def plan_keep(self):
        """``(keep, fill)`` of a keep plan (pa_plan_keep), else None."""
        n = 8
        lo, hi, fill = (I64 * n)(), (I64 * n)(), ctypes.c_int()
        if not self.lib.pa_plan_keep(self._plan, lo, hi, ctypes.byref(fill)):
            return None
        nk = len(self.keep) if self.keep is not None else 0
        return (tuple((int(lo[d]), int(hi[d])) for d in range(nk)),
                int(fill.value))

    def nsub(self, which: int, k: int = 0) -> int:
        return int(self.lib.pa_plan_nsub(self._plan, which, k))

    def copydesc_sub(self, n: int, f: int, which: int, k: int, s: int):
        nd = I64()
        dims = (I64 * 8)()
        sstr = (I64 * 8)()
        dstr = (I64 * 8)()
        soff = I64()
        doff = I64()
        st = self.lib.pa_plan_copydesc_sub(
            self._plan, n, f, which, k, s, ctypes.byref(nd), dims, sstr,
            ctypes.byref(soff), dstr, ctypes.byref(doff))
        if st != 0:
            return None
        m = nd.value
        return (tuple(dims[:m]), tuple(sstr[:m]), soff.value,
                tuple(dstr[:m]), doff.value)

    def nfill(self) -> int:
        return int(self.lib.pa_plan_nfill(self._plan))

    def filldesc(self, i: int):
        nd = I64()
        dims = (I64 * 8)()
        dstr = (I64 * 8)()
        doff = I64()
        _check(self.lib, self.lib.pa_plan_filldesc(
            self._plan, i, ctypes.byref(nd), dims, dstr, ctypes.byref(doff)),
            "pa_plan_filldesc")
        m = nd.value
        return (tuple(dims[:m]), tuple(dstr[:m]), doff.value)

    # ---- multi-field transposes (pa_*_many) ----------------------------

    @staticmethod
    def _ptrs(ptrs, n):
        if ptrs is None:
            return None
        if len(ptrs) != n:
            raise ValueError(f"expected {n} pointers, got {len(ptrs)}")
        return (VP * n)(*[VP(int(q)) for q in ptrs])

    def buffer_sizes_many(self, n: int) -> Tuple[int, int]:
        s, r = I64(), I64()
        _check(self.lib, self.lib.pa_plan_buffer_sizes_many(
            self._plan, n, ctypes.byref(s), ctypes.byref(r)),
            "pa_plan_buffer_sizes_many")
        return s.value, r.value

    def peer_message(self, n: int, k: int) -> Tuple[int, int, int, int]:
        """(send_off, send_bytes, recv_off, recv_bytes) of the one message
        exchanged with peer ``k`` for ``n`` fields."""
        out = (I64 * 4)()
        _check(self.lib, self.lib.pa_plan_peer_message(self._plan, n, k, out),
               "pa_plan_peer_message")
        return tuple(int(v) for v in out)

    def pack_many(self, src_ptrs, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_pack_many(
            self._plan, n, self._ptrs(src_ptrs, n), VP(stream)),
            "pa_transpose_pack_many")

    def local_many(self, src_ptrs, dst_ptrs, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_local_many(
            self._plan, n, self._ptrs(src_ptrs, n), self._ptrs(dst_ptrs, n),
            VP(stream)), "pa_transpose_local_many")

    def unpack_many(self, dst_ptrs, stream: int = 0):
        n = len(dst_ptrs)
        _check(self.lib, self.lib.pa_transpose_unpack_many(
            self._plan, n, self._ptrs(dst_ptrs, n), VP(stream)),
            "pa_transpose_unpack_many")

    def execute_many(self, src_ptrs, dst_ptrs, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_execute_many(
            self._plan, n, self._ptrs(src_ptrs, n), self._ptrs(dst_ptrs, n),
            VP(stream)), "pa_transpose_execute_many")

    # split and join transposes: ``n`` components on an ordinary scalar plan

    def pack_split(self, n: int, src_aos_ptr: int, stream: int = 0):
        _check(self.lib, self.lib.pa_transpose_pack_split(
            self._plan, n, VP(src_aos_ptr), VP(stream)),
            "pa_transpose_pack_split")

    def local_split(self, src_aos_ptr: int, dst_ptrs, stream: int = 0):
        n = len(dst_ptrs)
        _check(self.lib, self.lib.pa_transpose_local_split(
            self._plan, n, VP(src_aos_ptr), self._ptrs(dst_ptrs, n),
            VP(stream)), "pa_transpose_local_split")

    def local_join(self, src_ptrs, dst_aos_ptr: int, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_local_join(
            self._plan, n, self._ptrs(src_ptrs, n), VP(dst_aos_ptr),
            VP(stream)), "pa_transpose_local_join")

    def unpack_join(self, n: int, dst_aos_ptr: int, stream: int = 0):
        _check(self.lib, self.lib.pa_transpose_unpack_join(
            self._plan, n, VP(dst_aos_ptr), VP(stream)),
            "pa_transpose_unpack_join")

    def execute_split(self, src_aos_ptr: int, dst_ptrs, stream: int = 0):
        n = len(dst_ptrs)
        _check(self.lib, self.lib.pa_transpose_execute_split(
            self._plan, n, VP(src_aos_ptr), self._ptrs(dst_ptrs, n),
            VP(stream)), "pa_transpose_execute_split")

    def execute_join(self, src_ptrs, dst_aos_ptr: int, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_execute_join(
            self._plan, n, self._ptrs(src_ptrs, n), VP(dst_aos_ptr),
            VP(stream)), "pa_transpose_execute_join")

    # the same with a scale given per call: every real scalar of type
    # ``scalar`` (SCALAR_F32 / SCALAR_F64) times ``S(alpha)``, a split in its
    # pack and local copy, a join in its local copy and unpack

    def pack_split_scaled(self, n: int, scalar: int, alpha: float,
                          src_aos_ptr: int, stream: int = 0):
        _check(self.lib, self.lib.pa_transpose_pack_split_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            VP(src_aos_ptr), VP(stream)), "pa_transpose_pack_split_scaled")

    def local_split_scaled(self, scalar: int, alpha: float, src_aos_ptr: int,
                           dst_ptrs, stream: int = 0):
        n = len(dst_ptrs)
        _check(self.lib, self.lib.pa_transpose_local_split_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            VP(src_aos_ptr), self._ptrs(dst_ptrs, n), VP(stream)),
            "pa_transpose_local_split_scaled")

    def local_join_scaled(self, scalar: int, alpha: float, src_ptrs,
                          dst_aos_ptr: int, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_local_join_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            self._ptrs(src_ptrs, n), VP(dst_aos_ptr), VP(stream)),
            "pa_transpose_local_join_scaled")

    def unpack_join_scaled(self, n: int, scalar: int, alpha: float,
                           dst_aos_ptr: int, stream: int = 0):
        _check(self.lib, self.lib.pa_transpose_unpack_join_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            VP(dst_aos_ptr), VP(stream)), "pa_transpose_unpack_join_scaled")

    def execute_split_scaled(self, scalar: int, alpha: float,
                             src_aos_ptr: int, dst_ptrs, stream: int = 0):
        n = len(dst_ptrs)
        _check(self.lib, self.lib.pa_transpose_execute_split_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            VP(src_aos_ptr), self._ptrs(dst_ptrs, n), VP(stream)),
            "pa_transpose_execute_split_scaled")

    def execute_join_scaled(self, scalar: int, alpha: float, src_ptrs,
                            dst_aos_ptr: int, stream: int = 0):
        n = len(src_ptrs)
        _check(self.lib, self.lib.pa_transpose_execute_join_scaled(
            self._plan, n, int(scalar), ctypes.c_double(alpha),
            self._ptrs(src_ptrs, n), VP(dst_aos_ptr), VP(stream)),
            "pa_transpose_execute_join_scaled")

    def stage_table_count(self) -> int:
        """Stage tables in the plan's cache (pa_plan_stage_table_count)."""
        return int(self.lib.pa_plan_stage_table_count(self._plan))

    def stage_table_builds(self) -> int:
        """Stage tables built so far, evicted ones included
        (pa_plan_stage_table_builds)."""
        return int(self.lib.pa_plan_stage_table_builds(self._plan))

    def copydesc_many(self, n: int, f: int, which: int, k: int = 0):
        nd = I64()
        dims = (I64 * 8)()
        sstr = (I64 * 8)()
        dstr = (I64 * 8)()
        soff = I64()
        doff = I64()
        st = self.lib.pa_plan_copydesc_many(
            self._plan, n, f, which, k, ctypes.byref(nd), dims, sstr,
            ctypes.byref(soff), dstr, ctypes.byref(doff))
        if st != 0:
            return None
        m = nd.value
        return (tuple(dims[:m]), tuple(sstr[:m]), soff.value,
                tuple(dstr[:m]), doff.value)

    def stage_launches(self, n: int, stage: int, src_ptrs=None,
                       dst_ptrs=None):
        """The launches stage ``stage`` (STAGE_PACK / STAGE_LOCAL /
        STAGE_UNPACK) makes for ``n`` fields: a list of
        :class:`StageLaunch`.  Host-only; pointers (optional) are used for
        alignment only."""
        cap = 64
        while True:
            rows = ((I64 * 4) * cap)()
            nrows = ctypes.c_int()
            _check(self.lib, self.lib.pa_plan_stage_launches(
                self._plan, n, stage, self._ptrs(src_ptrs, n),
                self._ptrs(dst_ptrs, n), cap, rows, ctypes.byref(nrows)),
                "pa_plan_stage_launches")
            if nrows.value <= cap:
                break
            cap = nrows.value
        return [StageLaunch(int(r[0]), bool(r[1]), int(r[2]), int(r[3]))
                for r in rows[:nrows.value]]

    def stage_launches_soa(self, n: int, direction: int, stage: int,
                           aos_ptr: int = 0, field_ptrs=None):
        """The launches a split / join stage makes for ``n`` components
        (pa_plan_stage_launches_soa): ``direction`` SOA_SPLIT or SOA_JOIN,
        ``stage`` the pack or local stage of a split, the local or unpack
        stage of a join.  A list of :class:`StageLaunch`.  Host-only;
        pointers (optional) are used for alignment only."""
        cap = 64
        while True:
            rows = ((I64 * 4) * cap)()
            nrows = ctypes.c_int()
            _check(self.lib, self.lib.pa_plan_stage_launches_soa(
                self._plan, n, direction, stage, VP(aos_ptr or None),
                self._ptrs(field_ptrs, n), cap, rows, ctypes.byref(nrows)),
                "pa_plan_stage_launches_soa")
            if nrows.value <= cap:
                break
            cap = nrows.value
        return [StageLaunch(int(r[0]), bool(r[1]), int(r[2]), int(r[3]))
                for r in rows[:nrows.value]]

    def __del__(self):
        lib = getattr(self, "lib", None)
        if lib is None:
            return
        if getattr(self, "_plan", None):
            lib.pa_plan_destroy(self._plan)
        for h in (getattr(self, "_pi", None), getattr(self, "_po", None)):
            if h:
                lib.pa_pencil_destroy(h)
        if getattr(self, "_topo", None):
            lib.pa_topology_destroy(self._topo)


class NativeComm:
    def __init__(self, handle):
        self.handle = handle

    @classmethod
    def create(cls, uid: bytes, nranks: int, rank: int) -> "NativeComm":
        lib = load()
        h = VP()
        _check(lib, lib.pa_comm_create(
            ctypes.create_string_buffer(uid, len(uid)), nranks, rank,
            ctypes.byref(h)), "pa_comm_create")
        return cls(h)


_COMM_CACHE: Dict[tuple, NativeComm] = {}


def exchange_uid(topology, r_dim, rank: int, uid_fn) -> Tuple[bytes, int, int]:
    """Exchange the subgroup's RCCL unique id through the torch.distributed
    store: the subgroup leader (coordinate 0 along r_dim) generates it with
    ``uid_fn()`` and publishes it under a key unique to the subgroup; the
    others fetch it, acknowledge, and the leader deletes the key — so a
    reused store (restart, comm re-creation) can never serve a stale uid.
    ``r_dim=None`` means the FULL topology (the world communicator used by
    reductions).  Returns (uid, subgroup_size, subgroup_rank).
    Assumes dist rank == topology rank (one process per GPU)."""
    if r_dim is None:
        ranks = list(range(topology.nranks))
    else:
        ranks = topology.subgroup_ranks(rank, r_dim)
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError(
            "multi-GPU transpose needs torch.distributed initialised for the "
            "RCCL unique-id exchange")
    if dist.get_world_size() != topology.nranks:
        raise RuntimeError(
            f"torch.distributed world size {dist.get_world_size()} != "
            f"topology nranks {topology.nranks} (one process per GPU, dist "
            f"rank == topology rank)")
    if dist.get_rank() != rank:
        raise RuntimeError(
            f"torch.distributed rank {dist.get_rank()} != topology rank "
            f"{rank}")
    store = dist.distributed_c10d._get_default_store()
    sub_rank = ranks.index(rank)
    store_key = f"pencilhip_uid_{topology.dims}_{r_dim}_{min(ranks)}"
    ack_key = store_key + "_ack"
    if sub_rank == 0:
        uid = uid_fn()
        store.set(store_key, uid)
        # wait until every follower has read the uid, then retire the key
        import time as _time
        while store.add(ack_key, 0) < len(ranks) - 1:
            _time.sleep(0.001)
        try:
            store.delete_key(store_key)
            store.delete_key(ack_key)
        except Exception:
            pass  # stores without delete_key: keys stay (benign in-session)
    else:
        uid = bytes(store.get(store_key))
        store.add(ack_key, 1)
    return uid, len(ranks), sub_rank


def _nccl_uid() -> bytes:
    lib = load()
    n = lib.pa_unique_id_size()
    buf = ctypes.create_string_buffer(n)
    _check(lib, lib.pa_get_unique_id(buf), "pa_get_unique_id")
    return bytes(buf.raw)


def subgroup_comm(topology, r_dim: int, rank: int) -> Optional[NativeComm]:
    """RCCL communicator for the 1-D subgroup through ``rank`` along
    ``r_dim`` (replacing topology.subcomms[R], MPITopologies.jl:244-251)."""
    ranks = topology.subgroup_ranks(rank, r_dim)
    if len(ranks) == 1:
        return None
    key = (tuple(topology.dims), r_dim, tuple(ranks))
    if key in _COMM_CACHE:
        return _COMM_CACHE[key]
    uid, nranks, sub_rank = exchange_uid(topology, r_dim, rank, _nccl_uid)
    comm = NativeComm.create(uid, nranks, sub_rank)
    _COMM_CACHE[key] = comm
    return comm


def world_comm(topology, rank: int) -> Optional[NativeComm]:
    """RCCL communicator over the FULL topology (every rank): the engine
    backend for reductions' single Allreduce (reductions.jl:17-18)."""
    if topology.nranks == 1:
        return None
    key = (tuple(topology.dims), None, topology.nranks)
    if key in _COMM_CACHE:
        return _COMM_CACHE[key]
    uid, nranks, sub_rank = exchange_uid(topology, None, rank, _nccl_uid)
    comm = NativeComm.create(uid, nranks, sub_rank)
    _COMM_CACHE[key] = comm
    return comm


def allreduce_tensor(comm: NativeComm, t, op: str):
    """In-place ncclAllReduce of a contiguous cuda tensor through the native
    engine (pa_allreduce; reductions.jl:17-18)."""
    import torch
    lib = load()
    dtmap = {torch.float64: 0, torch.float32: 1, torch.int64: 2,
             torch.int32: 3, torch.uint8: 4}
    opmap = {"sum": 0, "prod": 1, "min": 2, "max": 3}
    if t.dtype not in dtmap:
        raise TypeError(f"pa_allreduce: unsupported dtype {t.dtype}")
    stream = torch.cuda.current_stream().cuda_stream
    _check(lib, lib.pa_allreduce(
        comm.handle, VP(t.data_ptr()), VP(t.data_ptr()), I64(t.numel()),
        dtmap[t.dtype], opmap[op], VP(stream)), "pa_allreduce")
    return t


class StagingPool:
    """Per-device shared staging buffers — the engine's analogue of the
    reference's send_buf/recv_buf shared across derived pencils
    (Pencils.jl:187-189, 257-271; the JLArray test even asserts no
    reallocation, test/array_types.jl:118-127).  Grow-only; every
    NativeTransposition on the device slices the same two tensors, so an
    x->y->z chain holds ONE send/recv pair.  Safe for same-stream chaining
    (stream order serialises reuse), like the reference's shared buffers
    under deferred waits."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.device = device
        self.send = torch.empty(0, dtype=torch.uint8, device=device)
        self.recv = torch.empty(0, dtype=torch.uint8, device=device)
        self.version = 0

    def reserve(self, send_bytes: int, recv_bytes: int):
        grow = (send_bytes > self.send.numel()
                or recv_bytes > self.recv.numel())
        if grow:
            # growth is a plan-creation-time event; drain in-flight work
            # (incl. the engine's comm stream, invisible to torch) before
            # retiring the old buffers
            if self.device.type == "cuda":
                self.torch.cuda.synchronize(self.device)
            if send_bytes > self.send.numel():
                self.send = self.torch.empty(
                    send_bytes, dtype=self.torch.uint8, device=self.device)
            if recv_bytes > self.recv.numel():
                self.recv = self.torch.empty(
                    recv_bytes, dtype=self.torch.uint8, device=self.device)
            self.version += 1
        return self.send, self.recv


_POOLS: Dict[int, StagingPool] = {}


def staging_pool(device) -> StagingPool:
    idx = device.index if device.index is not None else 0
    if idx not in _POOLS:
        _POOLS[idx] = StagingPool(device)
    return _POOLS[idx]


def _native_plan_for(plan, src, pair, group_cvt: bool = False,
                     scale=None) -> NativePlan:
    """The native plan of a (Multi)Transposition over arrays like ``src``;
    ``pair`` is its wire.WirePair or None, ``group_cvt`` its
    ``wire_grouped``, ``scale`` its scale.Scale or None."""
    if pair is None:
        np_ = NativePlan(plan.Pi, plan.Po, plan.rank,
                         src.data.element_size(), plan.extra_dims,
                         aliased=plan.aliased, ncomp=src.ncomp,
                         keep=plan.keep, fill=plan.fill)
        if scale is not None:
            np_.set_scale(scale.code, scale.alpha)
        return np_
    if scale is not None:
        raise ValueError("scale together with a wire pair is not supported")
    return NativePlan(plan.Pi, plan.Po, plan.rank, pair.stored.itemsize,
                      plan.extra_dims, aliased=plan.aliased,
                      ncomp=src.ncomp * pair.comps, wire=pair.code,
                      group_cvt=group_cvt)


class NativeTransposition:
    """GPU execution of one Transposition: staging buffers from torch's
    allocator, kernels + RCCL inside the native library."""

    def __init__(self, t):
        import torch
        self.torch = torch
        plan = t.plan
        src = t.src
        self.np_plan = plan
        self.native = _native_plan_for(plan, src, getattr(t, "wire", None),
                                       getattr(t, "wire_grouped", False),
                                       getattr(t, "scale", None))
        sb, rb = self.native.buffer_sizes()
        dev = src.data.device
        # Staging comes from the per-device shared pool (the reference's
        # buffer sharing across derived pencils, Pencils.jl:257-271) unless
        # PENCILHIP_PRIVATE_STAGING=1 asks for plan-private buffers.
        # never hand the engine a null pointer (a null send_buf would
        # trigger its hipMalloc fallback and orphan the pool's recv buffer)
        self._need = (max(sb, 1), max(rb, 1))
        if os.environ.get("PENCILHIP_PRIVATE_STAGING") == "1":
            self._pool = None
            self._send = torch.empty(max(sb, 1), dtype=torch.uint8,
                                     device=dev)
            self._recv = torch.empty(max(rb, 1), dtype=torch.uint8,
                                     device=dev)
            self.native.set_buffers(self._send.data_ptr(),
                                    self._recv.data_ptr())
        else:
            self._pool = staging_pool(dev)
            self._bind_pool()
        if self.native.nproc_sub > 1:
            comm = subgroup_comm(plan.Pi.topology, self.native.r_dim,
                                 plan.rank)
            if comm is not None:
                self.native.set_comm(comm)

    def _bind_pool(self):
        send, recv = self._pool.reserve(*self._need)
        self._send, self._recv = send, recv
        self.native.set_buffers(send.data_ptr(), recv.data_ptr())
        self._pool_version = self._pool.version

    def execute(self, src_tensor, dst_tensor, sync: bool = True):
        torch = self.torch
        assert src_tensor.is_cuda and dst_tensor.is_cuda
        assert src_tensor.is_contiguous() and dst_tensor.is_contiguous()
        if self._pool is not None and \
                self._pool.version != self._pool_version:
            self._bind_pool()  # another plan grew the pool: re-point
        stream = torch.cuda.current_stream().cuda_stream
        self.native.execute(src_tensor.data_ptr(), dst_tensor.data_ptr(),
                            stream)
        if sync:
            self.native.wait(stream)


class NativeMultiTransposition:
    """GPU execution of one MultiTransposition: ``n`` fields of one pencil
    pair through ONE native plan (pa_transpose_execute_many).  Staging is
    ``n`` times the plan's sizes, reserved from the shared StagingPool and
    re-pointed when the pool grows, like NativeTransposition."""

    def __init__(self, mt):
        src = mt.srcs[0]
        self._setup(_native_plan_for(mt.plan, src, getattr(mt, "wire", None),
                                     getattr(mt, "wire_grouped", False),
                                     getattr(mt, "scale", None)),
                    mt.plan, len(mt.srcs), src.data.device)

    def _setup(self, native_plan: NativePlan, plan, n: int, dev):
        """Staging for ``n`` fields of ``native_plan`` on device ``dev`` and
        the subgroup communicator of ``plan`` (the Python plan it mirrors)."""
        import torch
        self.torch = torch
        self.n = n
        self.native = native_plan
        sb, rb = self.native.buffer_sizes_many(self.n)
        self._need = (max(sb, 1), max(rb, 1))
        if os.environ.get("PENCILHIP_PRIVATE_STAGING") == "1":
            self._pool = None
            self._send = torch.empty(self._need[0], dtype=torch.uint8,
                                     device=dev)
            self._recv = torch.empty(self._need[1], dtype=torch.uint8,
                                     device=dev)
            self.native.set_buffers(self._send.data_ptr(),
                                    self._recv.data_ptr())
        else:
            self._pool = staging_pool(dev)
            self._bind_pool()
        if self.native.nproc_sub > 1:
            comm = subgroup_comm(plan.Pi.topology, self.native.r_dim,
                                 plan.rank)
            if comm is not None:
                self.native.set_comm(comm)

    def _bind_pool(self):
        send, recv = self._pool.reserve(*self._need)
        if (getattr(self, "_send", None) is not send
                or getattr(self, "_recv", None) is not recv):
            # set_buffers drops the engine's stage tables, so only re-point
            # when the pool really handed out other tensors
            self._send, self._recv = send, recv
            self.native.set_buffers(send.data_ptr(), recv.data_ptr())
        self._pool_version = self._pool.version

    def execute(self, src_tensors, dst_tensors, sync: bool = True):
        torch = self.torch
        for t in list(src_tensors) + list(dst_tensors):
            assert t.is_cuda and t.is_contiguous()
        if self._pool is not None and \
                self._pool.version != self._pool_version:
            self._bind_pool()  # another plan grew the pool: re-point
        stream = torch.cuda.current_stream().cuda_stream
        self.native.execute_many([t.data_ptr() for t in src_tensors],
                                 [t.data_ptr() for t in dst_tensors], stream)
        if sync:
            self.native.wait(stream)


class NativeSoaTransposition(NativeMultiTransposition):
    """GPU execution of one SplitTransposition or JoinTransposition: the
    ordinary scalar native plan, the ``n``-field staging and the communicator
    of a MultiTransposition over the scalar fields, run with the
    vector-valued array on one side (pa_transpose_execute_split / _join).
    A scale of the transposition goes with every call
    (pa_transpose_execute_split_scaled / _join_scaled): the plan has none."""

    def __init__(self, t):
        plan, f0 = t.plan, t.fields[0]
        self._setup(NativePlan(plan.Pi, plan.Po, plan.rank,
                               f0.data.element_size(), plan.extra_dims,
                               keep=plan.keep, fill=plan.fill,
                               group_soa=getattr(t, "grouped", False)),
                    plan, t.n, f0.data.device)
        self.split = t.split
        self.scale = getattr(t, "scale", None)  # scale.Scale or None

    def execute(self, aos_tensor, field_tensors, sync: bool = True):
        torch = self.torch
        for t in [aos_tensor] + list(field_tensors):
            assert t.is_cuda and t.is_contiguous()
        if self._pool is not None and \
                self._pool.version != self._pool_version:
            self._bind_pool()  # another plan grew the pool: re-point
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [t.data_ptr() for t in field_tensors]
        s = self.scale
        if self.split and s is not None:
            self.native.execute_split_scaled(s.code, s.alpha,
                                             aos_tensor.data_ptr(), ptrs,
                                             stream)
        elif self.split:
            self.native.execute_split(aos_tensor.data_ptr(), ptrs, stream)
        elif s is not None:
            self.native.execute_join_scaled(s.code, s.alpha, ptrs,
                                            aos_tensor.data_ptr(), stream)
        else:
            self.native.execute_join(ptrs, aos_tensor.data_ptr(), stream)
        if sync:
            self.native.wait(stream)
