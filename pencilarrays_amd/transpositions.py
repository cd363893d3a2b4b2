"""transpose!: the global pencil redistribution (the hot path).

Host orchestration mirroring src/Transpositions/Transpositions.jl:

- ``Transposition(dest, src)`` — plan object (Transpositions.jl:94-119), here
  amortisable across calls (the reference re-plans per call, :165-167).
- ``transpose(t)`` / ``transpose_into(dest, src)`` — :142-180.

Execution backends:

- **numpy + torch.distributed (gloo or none)** — the host mirror used by CPU
  tests (including world_size>1 gloo runs, standing in for the reference's
  "N MPI ranks on one box" test harness, test/runtests.jl:29-54).  Pack /
  unpack / fused-local copies run the SAME CopyDescs as the GPU engine, via
  numpy.  Exchange uses isend/irecv pairs (tag 42, Transpositions.jl:469-477).
- **torch cuda tensors** — the product path: every copy and the RCCL exchange
  run inside the native HIP engine (`libpencilhip.so`).  If the native engine
  is unavailable this path raises — there is no silent eager fallback.
"""

from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np

from .array import PencilArray
from .copyexec import (apply_copy, apply_copy_conv, apply_copy_soa,
                       apply_fill)
from .pencil import Pencil
from .plan import (TransposePlan, build_plan, buffer_nelem_many,
                   peer_message, stage_descs)
from .plan import fourier_keep  # noqa: F401  (the keep-set helper, re-exported)
from .scale import resolve_scale, scale_array
from .wire import narrow, resolve_wire, widen

MPI_TAG = 42  # Transpositions.jl:469


def _wire(buf: np.ndarray):
    """A staging-buffer slice as a torch tensor for isend/irecv: elements of
    any kind (opaque, wire scalars) travel as their bytes."""
    import torch
    return torch.from_numpy(buf.view(np.uint8))


def _wire_pair(dest: PencilArray, src: PencilArray, wire_dtype):
    """The wire pair of a transpose ``dest <- src`` sent as ``wire_dtype``
    (ValueError where the engine has none), or None."""
    if wire_dtype is None:
        return None
    pair = resolve_wire(src.data.dtype, wire_dtype)
    if str(dest.data.dtype) != str(src.data.dtype):
        raise ValueError(
            f"a reduced-precision wire needs dest and src of one dtype: "
            f"{dest.data.dtype} != {src.data.dtype}")
    return pair


def _check_keep_wire(keep, wire_dtype):
    if keep is not None and wire_dtype is not None:
        raise ValueError(
            "keep together with wire_dtype is not supported: a truncated "
            "transpose moves the stored type")


def _scale_of(dest: PencilArray, src: PencilArray, scale, wire_dtype):
    """The scale.Scale of a transpose ``dest <- scale * src`` (ValueError for
    a dtype or value the engine refuses, or together with a wire), or None
    for no scale."""
    if scale is None:
        return None
    if wire_dtype is not None:
        raise ValueError(
            "scale together with wire_dtype is not supported: that would be "
            "two roundings per element")
    if str(dest.data.dtype) != str(src.data.dtype):
        raise ValueError(
            f"a scaled transpose needs dest and src of one dtype: "
            f"{dest.data.dtype} != {src.data.dtype}")
    return resolve_scale(src.data.dtype, scale)


def _check_wire_grouped(wire_grouped, wire_dtype):
    if wire_grouped and wire_dtype is None:
        raise ValueError(
            "wire_grouped=True needs a wire_dtype: it groups the converting "
            "kernels of a reduced-precision wire")


class _Codec(NamedTuple):
    """The two things in which the host mirror of a reduced-precision wire
    differs from the plain one: how an array and the staging buffers are
    typed, and the copy that runs a descriptor."""
    view: Callable        # PencilArray -> the flat array descriptors index
    carrier: Optional[np.dtype]  # staging dtype; None = that of the view
    scale: int            # staging scalars per element
    copy: Callable        # (which, desc, src, dst): run one descriptor


def _codec(src: PencilArray, pair, scale=None) -> _Codec:
    if scale is not None:
        # scaled: typed real scalars; the local copy, the self unpack and
        # the unpacks multiply, the packs move the scalars as they are
        nc = src.ncomp * scale.comps  # real scalars per element
        a = scale.a

        def mul(x):
            with np.errstate(all="ignore"):
                return x * a

        conv = {0: mul, 1: lambda x: x, 2: mul, 3: lambda x: x, 4: mul}
        return _Codec(lambda arr: arr.data.view(scale.real), None, nc,
                      lambda which, d, s, t: apply_copy_conv(d, s, t, nc,
                                                             conv[which]))
    if pair is None:
        # plain elements: one opaque item per element (vector-valued ones
        # included), so the element-unit descriptors apply unchanged
        return _Codec(lambda a: a.element_view(), None, 1,
                      lambda which, d, s, t: apply_copy(d, s, t))
    # wire: packs narrow, unpacks widen, the local copy rounds
    nc = src.ncomp * pair.comps  # stored scalars per element
    conv = {0: lambda x: widen(narrow(x, pair), pair),
            1: lambda x: narrow(x, pair), 2: lambda w: widen(w, pair)}
    conv[3], conv[4] = conv[1], conv[2]  # the staged self block likewise
    return _Codec(lambda a: a.data.view(pair.stored), pair.carrier, nc,
                  lambda which, d, s, t: apply_copy_conv(d, s, t, nc,
                                                         conv[which]))


def _dist_for(plan: TransposePlan, use_dist: bool):
    """torch.distributed for the exchange of ``plan``: one process per rank,
    so its rank and world must be the topology's (a mismatch would silently
    address the wrong peers)."""
    if not use_dist:
        raise RuntimeError(
            "distributed transpose requires torch.distributed to be "
            "initialised (or use run_transpose_sim for in-process tests)")
    import torch.distributed as dist
    topo = plan.Pi.topology
    if dist.get_world_size() != topo.nranks:
        raise RuntimeError(
            f"torch.distributed world size {dist.get_world_size()} != "
            f"topology nranks {topo.nranks}")
    if dist.get_rank() != plan.rank:
        raise RuntimeError(
            f"torch.distributed rank {dist.get_rank()} != topology "
            f"rank {plan.rank}")
    return dist


def _arrays_alias(a, b) -> bool:
    """Base.mightalias equivalent (Transpositions.jl:250): do the two parent
    buffers share memory?  (ManyPencilArray in-place transposes.)"""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return np.shares_memory(a, b)
    if not isinstance(a, np.ndarray) and not isinstance(b, np.ndarray):
        try:
            sa, sb = a.untyped_storage(), b.untyped_storage()
            if sa.data_ptr() != sb.data_ptr():
                # conservative overlap check on address ranges
                a0, a1 = a.data_ptr(), a.data_ptr() + a.nbytes
                b0, b1 = b.data_ptr(), b.data_ptr() + b.nbytes
                return a0 < b1 and b0 < a1
            return True
        except Exception:
            return False
    return False


class Transposition:
    def __init__(self, dest: PencilArray, src: PencilArray,
                 method: str = "grouped", wire_dtype=None, keep=None,
                 fill="zero", wire_grouped: bool = False, scale=None):
        """``Transposition(Ao, Ai; method)`` (Transpositions.jl:94-119).

        ``scale`` (a finite real number) makes this a scaled transpose,
        ``dest = scale * T(src)``: every real scalar of float32 / float64 /
        complex64 / complex128 arrays (a complex item component by component)
        is multiplied once by ``scale`` rounded to the scalar type, in the
        pass that writes ``dest`` -- the local copy and the unpacks; messages
        carry unscaled bytes (pa_plan_set_scale).  The normalisation of an
        inverse FFT without a pass of its own.  ``None`` and ``1.0`` mean no
        scale.  Works with ``keep``; not available with ``wire_dtype``.

        ``keep`` (``(a, b)`` per logical dim, ``None`` entries meaning full;
        see :func:`fourier_keep`) makes this a truncated transpose: only
        global indices with ``i_d < a_d`` or ``i_d >= N_d - b_d`` in every
        dim move, bit for bit; the rest of ``dest`` becomes +0 with
        ``fill="zero"`` and is left untouched with ``fill=None``
        (pa_plan_create_keep).  Not available together with ``wire_dtype``.

        ``wire_dtype`` (``"float32"``, ``"float16"``, ``"bfloat16"``, or the
        numpy / torch dtype) sends the data in that narrower real scalar type:
        packs narrow, unpacks widen, the local copy rounds, so that
        ``dest == T(round_wire(src))`` whatever the process grid
        (pa_plan_create_wire).  complex128 with float32 is complex64 on the
        wire.  ``None`` moves the bytes as they are.

        ``wire_grouped=True`` (only with ``wire_dtype``) runs the converting
        kernels of each stage as grouped launches on the GPU
        (PA_PLAN_GROUP_CVT); the result is the same bit for bit, and the
        numpy host mirror, which has no launches, ignores it.

        ``method`` is accepted for signature parity with the reference's
        PointToPoint/Alltoallv choice (:56-68): on MI355X both map to the
        same grouped ncclSend/ncclRecv exchange over xGMI (RCCL has no
        alltoallv; grouped p2p IS the alltoall realisation), so the value
        ("grouped", "point_to_point", "alltoallv") does not change the
        execution.
        """
        if dest.extra_dims != src.extra_dims:
            raise ValueError(
                f"incompatible number of extra dimensions of PencilArrays: "
                f"{src.extra_dims} != {dest.extra_dims}")
        if dest.elem_dims != src.elem_dims:
            raise ValueError(
                f"incompatible element dimensions of PencilArrays: "
                f"{src.elem_dims} != {dest.elem_dims}")
        if dest.rank != src.rank:
            raise ValueError("dest and src must live on the same rank")
        if method not in ("grouped", "point_to_point", "alltoallv"):
            raise ValueError(f"unknown transpose method {method!r}")
        _check_keep_wire(keep, wire_dtype)
        _check_wire_grouped(wire_grouped, wire_dtype)
        self.method = method
        self.wire = _wire_pair(dest, src, wire_dtype)
        self.wire_grouped = bool(wire_grouped)
        self.scale = _scale_of(dest, src, scale, wire_dtype)
        self.src = src
        self.dest = dest
        self.aliased = _arrays_alias(src.data, dest.data)
        self.plan: TransposePlan = build_plan(
            src.pencil, dest.pencil, src.rank, src.extra_dims,
            aliased=self.aliased, keep=keep, fill=fill)
        self._native = None  # set lazily for the GPU path

    # ------------------------------------------------------------------
    # CPU (numpy) execution — host mirror / test infrastructure.
    # ------------------------------------------------------------------

    def _execute_numpy(self, use_dist: bool):
        """Every stage of any plan through ``stage_descs``: one copy per
        sub-block, one message per peer of the elements that move, the zero
        fill of a keep plan next to the local copy."""
        plan = self.plan
        codec = _codec(self.src, self.wire, self.scale)
        src, dst = codec.view(self.src), codec.view(self.dest)
        dt, sc = codec.carrier or src.dtype, codec.scale
        send_buf = np.empty(plan.send_nelem_total * sc, dtype=dt)
        recv_buf = np.empty(plan.recv_nelem_total * sc, dtype=dt)

        # 1. pack all remote blocks (Transpositions.jl:346-431); in aliased
        # mode also stage the self block into the recv tail BEFORE any write
        # of dst (:394-404)
        for which, d in stage_descs(plan, 1, 0, 0):
            codec.copy(which, d, src, send_buf if which == 1 else recv_buf)

        # 2. exchange: per-peer nonblocking send/recv (:463-479); a peer with
        # nothing kept is absent from it.  An ordinary plan asks for the
        # process group whenever its subgroup has peers.
        reqs = []
        msgs = [blk for blk in plan.peers if blk.peer_k != plan.my_k
                and (blk.send_nelem or blk.recv_nelem)]
        if msgs or (plan.keep is None and plan.nproc_sub > 1):
            dist = _dist_for(plan, use_dist)
            for blk in msgs:
                if blk.recv_nelem > 0:
                    rt = _wire(recv_buf[blk.recv_offset * sc:
                                        (blk.recv_offset + blk.recv_nelem) * sc])
                    reqs.append(dist.irecv(rt, src=blk.global_rank,
                                           tag=MPI_TAG))
                if blk.send_nelem > 0:
                    st = _wire(send_buf[blk.send_offset * sc:
                                        (blk.send_offset + blk.send_nelem) * sc])
                    reqs.append(dist.isend(st, dst=blk.global_rank,
                                           tag=MPI_TAG))

        # 3. fused local (self) block overlaps the exchange (:394-404 + :530)
        for which, d in stage_descs(plan, 1, 0, 1):
            codec.copy(which, d, src if which == 0 else recv_buf, dst)
        for fd in plan.fills:  # element units, whatever the codec's view
            apply_fill(fd, self.dest.element_view())
        for r in reqs:
            r.wait()

        # 4. unpack received blocks (:489-536)
        for which, d in stage_descs(plan, 1, 0, 2):
            codec.copy(which, d, recv_buf, dst)

    # ------------------------------------------------------------------
    # GPU execution — native HIP engine only.
    # ------------------------------------------------------------------

    def _execute_torch_cuda(self, sync: bool):
        from . import native
        if self._native is None:
            self._native = native.NativeTransposition(self)
        self._native.execute(self.src.data, self.dest.data, sync=sync)

    # ------------------------------------------------------------------

    def execute(self, sync: bool = True):
        """Run the transpose.  ``sync=False`` is the reference's
        ``transpose!(t; waitall=false)`` contract (Transpositions.jl:142-158):
        the call returns with work enqueued on the stream; call :meth:`wait`
        (== ``MPI.Waitall(t)``, :128-131) before reusing the source or
        relying on the destination outside the stream."""
        if self.src.is_torch:
            if not self.src.data.is_cuda:
                raise RuntimeError(
                    "torch CPU tensors are not a supported backend: use "
                    "numpy arrays for the CPU host mirror, or cuda tensors "
                    "for the native engine")
            self._execute_torch_cuda(sync)
        else:
            import torch.distributed as dist
            self._execute_numpy(use_dist=dist.is_available() and dist.is_initialized())
        return self.dest

    def wait(self):
        """MPI.Waitall(t) (Transpositions.jl:128-131)."""
        if self._native is not None:
            import torch
            self._native.native.wait(torch.cuda.current_stream().cuda_stream)
        return self


def transpose_into(dest: PencilArray, src: PencilArray,
                   method: str = "grouped", wire_dtype=None, keep=None,
                   fill="zero", wire_grouped: bool = False,
                   scale=None) -> PencilArray:
    """``transpose!(dest, src; method)`` (Transpositions.jl:161-169)."""
    _check_wire_grouped(wire_grouped, wire_dtype)
    if dest is src:
        return dest
    return Transposition(dest, src, method=method, wire_dtype=wire_dtype,
                         keep=keep, fill=fill, wire_grouped=wire_grouped,
                         scale=scale).execute()


class MultiTransposition:
    """``n`` separately allocated fields of ONE pencil pair transposed in one
    call: ``MultiTransposition(dests, srcs)``, pair ``i`` being
    ``dests[i] <- srcs[i]``.  What a host does with ``n`` ``transpose!``
    calls (Transpositions.jl:161-180), as one plan: on the GPU one grouped
    kernel launch per stage and one message per peer carrying all fields
    (pa_transpose_execute_many).

    Every pair must have the same input pencil, output pencil, rank, element
    size, ``extra_dims``, ``elem_dims`` and device.  If any source aliases
    any destination (in-place pairs, or one pair's destination over another
    pair's source) the plan is aliased: every read of a source is enqueued
    before any write of a destination.

    numpy arrays run the host mirror — one single-field Transposition per
    field, which pins the semantics, not the performance.

    ``wire_dtype``: a reduced-precision wire for every field, as in
    :class:`Transposition`; ``wire_grouped``: its converting kernels as
    grouped launches, likewise.  ``keep`` / ``fill``: a truncated transpose of
    every field, as in :class:`Transposition`.  ``scale``: one factor for
    every field, likewise."""

    def __init__(self, dests: Sequence[PencilArray],
                 srcs: Sequence[PencilArray], wire_dtype=None, keep=None,
                 fill="zero", wire_grouped: bool = False, scale=None):
        _check_keep_wire(keep, wire_dtype)
        _check_wire_grouped(wire_grouped, wire_dtype)
        dests, srcs = list(dests), list(srcs)
        if len(dests) != len(srcs):
            raise ValueError(
                f"dests and srcs must have the same length: "
                f"{len(dests)} != {len(srcs)}")
        if not srcs:
            raise ValueError("MultiTransposition needs at least one field")
        s0, d0 = srcs[0], dests[0]

        def same_pencil(a, b):
            return (tuple(a.topology.dims) == tuple(b.topology.dims)
                    and tuple(a.size_global) == tuple(b.size_global)
                    and tuple(a.decomp_dims) == tuple(b.decomp_dims)
                    and tuple(a.perm) == tuple(b.perm))

        def storage(a):
            if a.is_torch:
                return ("torch", a.data.dtype, str(a.data.device))
            return ("numpy", a.data.dtype, "cpu")

        for i, (d, s) in enumerate(zip(dests, srcs)):
            if d.extra_dims != s.extra_dims or s.extra_dims != s0.extra_dims:
                raise ValueError(
                    f"field {i}: incompatible extra dimensions of "
                    f"PencilArrays: {s.extra_dims}, {d.extra_dims} != "
                    f"{s0.extra_dims}")
            if d.elem_dims != s.elem_dims or s.elem_dims != s0.elem_dims:
                raise ValueError(
                    f"field {i}: incompatible element dimensions of "
                    f"PencilArrays: {s.elem_dims}, {d.elem_dims} != "
                    f"{s0.elem_dims}")
            if d.rank != s.rank or s.rank != s0.rank:
                raise ValueError(
                    f"field {i}: every array must live on the same rank")
            if not same_pencil(s.pencil, s0.pencil):
                raise ValueError(
                    f"field {i}: source pencil differs from field 0's")
            if not same_pencil(d.pencil, d0.pencil):
                raise ValueError(
                    f"field {i}: destination pencil differs from field 0's")
            if storage(s) != storage(s0) or storage(d) != storage(s0):
                raise ValueError(
                    f"field {i}: every array must have the same backend, "
                    f"dtype and device: {storage(s)}, {storage(d)} != "
                    f"{storage(s0)}")
        self.srcs = srcs
        self.dests = dests
        self.wire_dtype = wire_dtype
        self.wire_grouped = bool(wire_grouped)
        self.keep, self.fill = keep, fill
        self.wire = _wire_pair(d0, s0, wire_dtype)
        self.scale = _scale_of(d0, s0, scale, wire_dtype)
        self.aliased = any(_arrays_alias(s.data, d.data)
                           for s in srcs for d in dests)
        self.plan: TransposePlan = build_plan(
            s0.pencil, d0.pencil, s0.rank, s0.extra_dims,
            aliased=self.aliased, keep=keep, fill=fill)
        self._native = None

    def _execute_numpy(self):
        if self.aliased and len(self.srcs) > 1:
            # a destination may overlap ANOTHER pair's source: read every
            # source before any destination is written
            srcs = [PencilArray(s.pencil, s.rank, s.data.copy(),
                                s.extra_dims, s.elem_dims)
                    for s in self.srcs]
        else:
            srcs = self.srcs
        for d, s in zip(self.dests, srcs):
            Transposition(d, s, wire_dtype=self.wire_dtype, keep=self.keep,
                          fill=self.fill, wire_grouped=self.wire_grouped,
                          scale=self.scale and self.scale.alpha).execute()

    def execute(self, sync: bool = True):
        """Run the transposes; ``sync=False`` returns with the work enqueued
        (see :meth:`Transposition.execute`)."""
        if self.srcs[0].is_torch:
            if not self.srcs[0].data.is_cuda:
                raise RuntimeError(
                    "torch CPU tensors are not a supported backend: use "
                    "numpy arrays for the CPU host mirror, or cuda tensors "
                    "for the native engine")
            from . import native
            if self._native is None:
                self._native = native.NativeMultiTransposition(self)
            self._native.execute([s.data for s in self.srcs],
                                 [d.data for d in self.dests], sync=sync)
        else:
            self._execute_numpy()
        return self.dests

    def wait(self):
        """MPI.Waitall(t) (Transpositions.jl:128-131)."""
        if self._native is not None:
            import torch
            self._native.native.wait(torch.cuda.current_stream().cuda_stream)
        return self


def transpose_many_into(dests: Sequence[PencilArray],
                        srcs: Sequence[PencilArray], wire_dtype=None,
                        keep=None, fill="zero", wire_grouped: bool = False,
                        scale=None):
    """``transpose!`` of every pair ``dests[i] <- srcs[i]`` in one call."""
    return MultiTransposition(dests, srcs, wire_dtype=wire_dtype, keep=keep,
                              fill=fill, wire_grouped=wire_grouped,
                              scale=scale).execute()


def _check_soa(aos: PencilArray, fields: Sequence[PencilArray]) -> int:
    """Validate the two sides of a split or join transpose (ValueError) and
    return ``n``: ``aos`` is the vector-valued array, ``fields`` its ``n``
    scalar fields on the other pencil."""
    fields = list(fields)
    n = len(fields)
    if n < 2:
        raise ValueError(
            f"a split or join transpose needs at least 2 fields (got {n})")
    if aos.ncomp != n or not aos.elem_dims:
        raise ValueError(
            f"the vector-valued array has {aos.ncomp} scalars per element "
            f"(elem_dims {aos.elem_dims}) for {n} fields")
    f0 = fields[0]

    def storage(a):
        if a.is_torch:
            return ("torch", a.data.dtype, str(a.data.device))
        return ("numpy", a.data.dtype, "cpu")

    def same_pencil(a, b):
        return (tuple(a.topology.dims) == tuple(b.topology.dims)
                and tuple(a.size_global) == tuple(b.size_global)
                and tuple(a.decomp_dims) == tuple(b.decomp_dims)
                and tuple(a.perm) == tuple(b.perm))

    for i, f in enumerate(fields):
        if f.elem_dims:
            raise ValueError(
                f"field {i}: a scalar field cannot have elem_dims "
                f"{f.elem_dims}")
        if f.extra_dims != aos.extra_dims:
            raise ValueError(
                f"field {i}: incompatible extra dimensions of PencilArrays: "
                f"{f.extra_dims} != {aos.extra_dims}")
        if f.rank != aos.rank:
            raise ValueError(
                f"field {i}: every array must live on the same rank")
        if not same_pencil(f.pencil, f0.pencil):
            raise ValueError(f"field {i}: pencil differs from field 0's")
        if storage(f) != storage(aos):
            raise ValueError(
                f"field {i}: the scalar dtype, backend and device must be "
                f"the same on both sides: {storage(f)} != {storage(aos)}")
        if _arrays_alias(f.data, aos.data) or any(
                _arrays_alias(f.data, g.data) for g in fields[:i]):
            raise ValueError(
                f"field {i}: a split or join transpose cannot run in place: "
                f"the arrays must not alias")
    if aos.data.dtype.itemsize not in (4, 8, 16):
        raise ValueError(
            f"a split or join transpose moves scalars of 4, 8 or 16 bytes, "
            f"not {aos.data.dtype}")
    return n


class _SoaTransposition:
    """What SplitTransposition and JoinTransposition share: ``aos`` is the
    vector-valued array, ``fields`` the scalar ones."""

    split: bool

    def __init__(self, aos: PencilArray, fields: Sequence[PencilArray],
                 scale=None, keep=None, fill="zero", grouped=None):
        self.aos, self.fields = aos, list(fields)
        self.n = _check_soa(aos, self.fields)
        # scale.Scale or None; None and 1.0 give the unscaled object
        self.scale = resolve_scale(aos.data.dtype, scale)
        self.keep, self.fill = keep, fill
        # grouped launches (PA_PLAN_GROUP_SOA) are what lets the native
        # stages run on a keep plan
        self.grouped = keep is not None if grouped is None else bool(grouped)
        if keep is not None and not self.grouped:
            raise ValueError(
                "keep needs grouped launches: a truncated split or join "
                "transpose cannot run with grouped=False")
        f0 = self.fields[0]
        Pi, Po = (aos.pencil, f0.pencil) if self.split else \
            (f0.pencil, aos.pencil)
        self.plan: TransposePlan = build_plan(Pi, Po, aos.rank,
                                              aos.extra_dims, keep=keep,
                                              fill=fill)
        self._native = None

    def _component(self, c: int) -> PencilArray:
        """Component ``c`` of the vector-valued array as a scalar array of
        its own (numpy)."""
        a = self.aos
        return PencilArray(a.pencil, a.rank,
                           np.ascontiguousarray(a.data.reshape(-1, self.n)[:, c]),
                           a.extra_dims)

    def _execute_numpy(self):
        # the host mirror pins the semantics, not the performance: one
        # single-field Transposition per component, which multiplies on the
        # real view (scale.py)
        alpha = self.scale and self.scale.alpha
        kw = dict(scale=alpha, keep=self.keep, fill=self.fill)
        if self.split:
            for c, f in enumerate(self.fields):
                Transposition(f, self._component(c), **kw).execute()
        else:
            for c, f in enumerate(self.fields):
                # the copy holds what the destination holds, which is what
                # fill=None leaves outside the keep set
                tmp = self._component(c)
                Transposition(tmp, f, **kw).execute()
                self.aos.data.reshape(-1, self.n)[:, c] = tmp.data

    def execute(self, sync: bool = True):
        """Run the transpose; ``sync=False`` returns with the work enqueued
        (see :meth:`Transposition.execute`)."""
        if self.aos.is_torch:
            if not self.aos.data.is_cuda:
                raise RuntimeError(
                    "torch CPU tensors are not a supported backend: use "
                    "numpy arrays for the CPU host mirror, or cuda tensors "
                    "for the native engine")
            from . import native
            if self._native is None:
                self._native = native.NativeSoaTransposition(self)
            self._native.execute(self.aos.data,
                                 [f.data for f in self.fields], sync=sync)
        else:
            self._execute_numpy()
        return self.fields if self.split else self.aos

    def wait(self):
        """MPI.Waitall(t) (Transpositions.jl:128-131)."""
        if self._native is not None:
            import torch
            self._native.native.wait(torch.cuda.current_stream().cuda_stream)
        return self


class SplitTransposition(_SoaTransposition):
    """``SplitTransposition(dests, src)``: the transpose that reads a
    vector-valued array writes scalar fields.  ``src`` has ``elem_dims`` of
    product ``n = len(dests)`` on the input pencil, every ``dests[c]`` is a
    scalar array of the same dtype on the output pencil, and
    ``dests[c] == T(src[c])`` bit for bit, component ``c`` being flat
    position ``c`` inside the element (pa_transpose_execute_split).  The
    layout change rides in the pack and the local copy; staging and messages
    are those of ``MultiTransposition`` on the component copies.

    ``scale`` (a finite real number; ``None`` and ``1.0`` mean none) makes it
    ``dests[c] == T(src[c] * scale)``: every real scalar of a float32 /
    float64 / complex64 / complex128 array (a complex item is two) is
    multiplied once by ``scale`` rounded to the scalar type, in the pack and
    the local copy, the two stages that carry the layout change
    (pa_transpose_execute_split_scaled).  Staging and messages therefore carry
    the SCALED scalars, those of ``MultiTransposition`` on the scaled component
    copies: the unpack is the ordinary one and cannot multiply.  Integer
    arrays take no scale (``ValueError``).

    ``keep`` / ``fill`` (as in :class:`Transposition`) make it a truncated
    split: only the elements of the keep set are moved,
    ``dests[c][i] == src[c][i]`` (times ``scale``) for ``i`` in the keep set,
    and outside it every destination reads ``+0`` (``fill="zero"``) or is
    left untouched (``fill=None``).  Staging and messages are those of
    ``MultiTransposition(keep=...)`` on the component copies.

    ``grouped``: run each stage as one grouped launch per kernel signature
    instead of one launch per block (PA_PLAN_GROUP_SOA); the result is the
    same bit for bit.  ``None`` means "exactly when ``keep`` is given": a
    keep plan needs the grouped stages, so ``keep`` with ``grouped=False``
    is a ``ValueError``."""

    split = True

    def __init__(self, dests: Sequence[PencilArray], src: PencilArray,
                 scale=None, keep=None, fill="zero", grouped=None):
        super().__init__(src, dests, scale, keep, fill, grouped)
        self.src, self.dests = src, self.fields


class JoinTransposition(_SoaTransposition):
    """``JoinTransposition(dest, srcs)``: the transpose that reads scalar
    fields writes the vector-valued array, ``dest[c] == T(srcs[c])`` bit for
    bit (pa_transpose_execute_join).  The layout change rides in the local
    copy and the unpack; see :class:`SplitTransposition`.

    ``scale`` makes it ``dest[c] == T(srcs[c] * scale)``, the ``1/N`` of an
    inverse FFT on the hop that writes the vector-valued physical-space array
    (pa_transpose_execute_join_scaled): the multiply sits in the local copy
    and the unpack, the destination side as in a scaled
    :class:`Transposition`, and staging and messages carry unscaled bytes,
    identical to the unscaled join's.

    ``keep`` / ``fill`` / ``grouped``: as in :class:`SplitTransposition`;
    the zero fill covers the whole elements of ``dest`` outside the keep
    set.  With ``keep``, ``fill="zero"`` and ``scale=1/N`` this is the
    inverse hop of a dealiased pseudo-spectral step."""

    split = False

    def __init__(self, dest: PencilArray, srcs: Sequence[PencilArray],
                 scale=None, keep=None, fill="zero", grouped=None):
        super().__init__(dest, srcs, scale, keep, fill, grouped)
        self.dest, self.srcs = dest, self.fields


def transpose_split_into(dests: Sequence[PencilArray], src: PencilArray,
                         scale=None, keep=None, fill="zero", grouped=None):
    """Split transpose ``dests[c] <- scale * src[c]`` in one call."""
    return SplitTransposition(dests, src, scale=scale, keep=keep, fill=fill,
                              grouped=grouped).execute()


def transpose_join_into(dest: PencilArray, srcs: Sequence[PencilArray],
                        scale=None, keep=None, fill="zero", grouped=None):
    """Join transpose ``dest[c] <- scale * srcs[c]`` in one call."""
    return JoinTransposition(dest, srcs, scale=scale, keep=keep, fill=fill,
                             grouped=grouped).execute()


# ----------------------------------------------------------------------
# In-process multi-rank simulation (test harness only): runs every rank's
# pack/exchange/unpack inside one process, memcpy standing in for the
# exchange.  This is how CPU tests cover P>1 without spawning processes.
# ----------------------------------------------------------------------

def run_transpose_sim(dests: Sequence[PencilArray],
                      srcs: Sequence[PencilArray],
                      staging_out=None, wire_dtype=None, keep=None,
                      fill="zero", wire_grouped: bool = False,
                      scale=None) -> None:
    """:func:`run_transpose_sim_many` with one field per rank (``n = 1`` is
    the single-field staging layout): ``dests[r] <- srcs[r]``."""
    return run_transpose_sim_many([[d] for d in dests], [[s] for s in srcs],
                                  staging_out, wire_dtype=wire_dtype,
                                  keep=keep, fill=fill,
                                  wire_grouped=wire_grouped, scale=scale)


def run_transpose_sim_many(dests_per_rank: Sequence[Sequence[PencilArray]],
                           srcs_per_rank: Sequence[Sequence[PencilArray]],
                           staging_out=None, wire_dtype=None, keep=None,
                           fill="zero", wire_grouped: bool = False,
                           scale=None) -> None:
    """Every rank's transpose of ``n`` fields with the multi-field staging
    layout (plan.py): every field of a rank is packed into ONE n-fold send
    buffer, and the exchange is ONE slice copy per peer pair of ``n * c``
    elements — the "one message per peer" contract.
    ``dests_per_rank[r][f]`` / ``srcs_per_rank[r][f]`` is field ``f`` on
    rank ``r``.  ``staging_out``, if a dict, receives the final
    ``send``/``recv`` buffers per rank (tests compare them).
    ``wire_dtype``: a reduced-precision wire (see :class:`Transposition`);
    the staging buffers then hold wire scalars (bfloat16 as uint16
    patterns), packs narrow, unpacks widen and the local copy rounds.
    ``keep`` / ``fill``: a truncated transpose; the staging buffers then hold
    the kept elements only, a peer pair with nothing kept copies nothing, and
    every field gets the zero fill.  ``wire_grouped`` is accepted for parity
    with :class:`Transposition`: the host mirror has no launches to group.
    ``scale``: a scaled transpose; the staging buffers then hold the real
    scalars of the unscaled elements, byte for byte those of the run without
    a scale, and the local copy and the unpacks multiply."""
    _check_keep_wire(keep, wire_dtype)
    _check_wire_grouped(wire_grouped, wire_dtype)
    nranks = len(srcs_per_rank)
    n = len(srcs_per_rank[0])
    if n < 1 or any(len(x) != n for x in srcs_per_rank) or \
            any(len(x) != n for x in dests_per_rank):
        raise ValueError("every rank needs the same number (>= 1) of fields")
    s00, d00 = srcs_per_rank[0][0], dests_per_rank[0][0]
    codec = _codec(s00, _wire_pair(d00, s00, wire_dtype),
                   _scale_of(d00, s00, scale, wire_dtype))
    plans = []
    for r in range(nranks):
        s0, d0 = srcs_per_rank[r][0], dests_per_rank[r][0]
        if d0.elem_dims != s0.elem_dims:
            raise ValueError(
                f"incompatible element dimensions of PencilArrays: "
                f"{s0.elem_dims} != {d0.elem_dims}")
        aliased = any(_arrays_alias(s.data, d.data)
                      for s in srcs_per_rank[r] for d in dests_per_rank[r])
        plans.append(build_plan(s0.pencil, d0.pencil, r, s0.extra_dims,
                                aliased=aliased, keep=keep, fill=fill))
    sflat = [[codec.view(s) for s in row] for row in srcs_per_rank]
    dflat = [[codec.view(d) for d in row] for row in dests_per_rank]
    dt, sc = codec.carrier or sflat[0][0].dtype, codec.scale
    send_bufs, recv_bufs = [], []
    for p in plans:
        ns, nr = buffer_nelem_many(p, n)
        send_bufs.append(np.empty(ns * sc, dtype=dt))
        recv_bufs.append(np.empty(nr * sc, dtype=dt))

    # pack every field on every rank (incl. staged self blocks) before any
    # destination is written
    for r, p in enumerate(plans):
        for f in range(n):
            for which, d in stage_descs(p, n, f, 0):
                codec.copy(which, d, sflat[r][f],
                           send_bufs[r] if which == 1 else recv_bufs[r])
    for r, p in enumerate(plans):
        for f in range(n):
            for which, d in stage_descs(p, n, f, 1):
                codec.copy(which, d,
                           sflat[r][f] if which == 0 else recv_bufs[r],
                           dflat[r][f])
            for fd in p.fills:  # element units, whatever the codec's view
                apply_fill(fd, dests_per_rank[r][f].element_view())

    # exchange: ONE slice copy per peer pair, all n fields in it
    for r, p in enumerate(plans):
        if p.r_dim is None:
            continue
        for blk in p.peers:
            if blk.peer_k == p.my_k or blk.send_nelem == 0:
                continue
            so, sn, _, _ = peer_message(p, n, blk.peer_k)
            # the matching recv block: the peer's block for MY coordinate
            q = plans[blk.global_rank]
            _, _, ro, rn = peer_message(q, n, p.my_k)
            assert rn == sn, (r, blk.peer_k, sn, rn)
            recv_bufs[blk.global_rank][ro * sc:(ro + rn) * sc] = \
                send_bufs[r][so * sc:(so + sn) * sc]

    # unpack every field on every rank
    for r, p in enumerate(plans):
        for f in range(n):
            for which, d in stage_descs(p, n, f, 2):
                codec.copy(which, d, recv_bufs[r], dflat[r][f])
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs


SIM_STAGES = ("pack", "exchange", "local", "unpack")


def _run_sim_soa(split: bool, aos_per_rank: Sequence[PencilArray],
                 fields_per_rank: Sequence[Sequence[PencilArray]],
                 staging_out=None, stages=SIM_STAGES,
                 staging_in=None, scale=None, keep=None,
                 fill="zero") -> None:
    """The multi-rank simulation of a split (``aos`` on the source pencil) or
    join (``aos`` on the destination pencil) transpose: the stages and the
    n-field staging layout of :func:`run_transpose_sim_many`, with the
    descriptors of one scalar component applied to the vector-valued side
    through ``apply_copy_soa``.  ``stages`` names the stages to run and
    ``staging_in`` supplies ``send`` / ``recv`` buffers, so that one side of
    a hop can be run by the ordinary n-field stages.  ``scale`` multiplies in
    the stages the engine multiplies in, on the real view of what the stage
    reads: a split's pack and local copy (staging holds scaled scalars), a
    join's local copy and unpack (staging holds unscaled ones).  ``keep`` /
    ``fill``: the plans are keep plans, so staging holds the kept elements
    only, and the local stage zero-fills the plan's fill windows: on every
    field of a split, on the whole elements of ``aos`` of a join."""
    unknown = set(stages) - set(SIM_STAGES)
    if unknown:
        raise ValueError(f"unknown stages {sorted(unknown)}")
    pack, local = "pack" in stages, "local" in stages
    exchange, unpack = "exchange" in stages, "unpack" in stages
    nranks = len(aos_per_rank)
    n = _check_soa(aos_per_rank[0], fields_per_rank[0])
    plans = []
    for r in range(nranks):
        a, fs = aos_per_rank[r], fields_per_rank[r]
        if _check_soa(a, fs) != n:
            raise ValueError("every rank needs the same number of fields")
        Pi, Po = (a.pencil, fs[0].pencil) if split else \
            (fs[0].pencil, a.pencil)
        plans.append(build_plan(Pi, Po, r, a.extra_dims, keep=keep,
                                fill=fill))
    dt = aos_per_rank[0].data.dtype
    sc = resolve_scale(dt, scale)

    def scaled(x):
        """What a multiplying stage reads: ``x (*) a``, or ``x`` itself."""
        return x if sc is None else scale_array(x, sc.alpha)

    if staging_in is not None:
        send_bufs, recv_bufs = staging_in["send"], staging_in["recv"]
    else:
        send_bufs, recv_bufs = [], []
        for p in plans:
            ns, nr = buffer_nelem_many(p, n)
            send_bufs.append(np.empty(ns, dtype=dt))
            recv_bufs.append(np.empty(nr, dtype=dt))

    for r, p in enumerate(plans):
        aos, fs = aos_per_rank[r].data, fields_per_rank[r]
        src_aos = scaled(aos) if split and (pack or local) else aos
        for c in range(n):
            if pack:
                for which, d in stage_descs(p, n, c, 0):
                    assert which == 1, "a split or join plan is not aliased"
                    if split:
                        apply_copy_soa(d, src_aos, send_bufs[r], n, c, True)
                    else:
                        apply_copy(d, fs[c].data, send_bufs[r])
            if local:
                for which, d in stage_descs(p, n, c, 1):
                    assert which == 0, "a split or join plan is not aliased"
                    if split:
                        apply_copy_soa(d, src_aos, fs[c].data, n, c, True)
                    else:
                        apply_copy_soa(d, aos, scaled(fs[c].data), n, c,
                                       False)
        if local:
            for fd in p.fills:  # element units: n scalars on the aos side
                if split:
                    for f in fs:
                        apply_fill(fd, f.element_view())
                else:
                    apply_fill(fd, aos_per_rank[r].element_view())

    # exchange: ONE slice copy per peer pair, all n components in it
    if exchange:
        for r, p in enumerate(plans):
            if p.r_dim is None:
                continue
            for blk in p.peers:
                if blk.peer_k == p.my_k or blk.send_nelem == 0:
                    continue
                so, sn, _, _ = peer_message(p, n, blk.peer_k)
                q = plans[blk.global_rank]
                _, _, ro, rn = peer_message(q, n, p.my_k)
                assert rn == sn, (r, blk.peer_k, sn, rn)
                recv_bufs[blk.global_rank][ro:ro + rn] = \
                    send_bufs[r][so:so + sn]

    if unpack:
        for r, p in enumerate(plans):
            aos, fs = aos_per_rank[r].data, fields_per_rank[r]
            src_recv = recv_bufs[r] if split else scaled(recv_bufs[r])
            for c in range(n):
                for which, d in stage_descs(p, n, c, 2):
                    if split:
                        apply_copy(d, recv_bufs[r], fs[c].data)
                    else:
                        apply_copy_soa(d, aos, src_recv, n, c, False)
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs


def run_transpose_sim_split(dests_per_rank: Sequence[Sequence[PencilArray]],
                            srcs: Sequence[PencilArray],
                            staging_out=None, stages=SIM_STAGES,
                            staging_in=None, scale=None, keep=None,
                            fill="zero") -> None:
    """Every rank's split transpose ``dests_per_rank[r][c] <- srcs[r][c]``
    (:class:`SplitTransposition`) with the n-field staging layout of
    :func:`run_transpose_sim_many`: the pack reads the vector-valued source
    and fills the ``n`` component slots of every send block, the exchange is
    one slice copy per peer pair, the unpack is the ordinary n-field one.
    ``staging_out``, if a dict, receives the ``send`` / ``recv`` buffers per
    rank, in scalars.  ``stages`` (a subset of ``SIM_STAGES``) runs only
    those stages, on the buffers of ``staging_in`` if given: the way to put
    an ordinary n-field stage on the other side of a hop.  ``scale``: the
    pack and the local copy multiply, so the buffers hold the SCALED scalars,
    byte for byte those of :func:`run_transpose_sim_many` on the scaled
    component copies, and the ordinary unpack delivers the scaled fields.
    ``keep`` / ``fill``: a truncated split, staging byte for byte that of
    :func:`run_transpose_sim_many` with the same ``keep``; the mirror has no
    launches, so there is no ``grouped`` here."""
    _run_sim_soa(True, srcs, dests_per_rank, staging_out, stages, staging_in,
                 scale, keep, fill)


def run_transpose_sim_join(dests: Sequence[PencilArray],
                           srcs_per_rank: Sequence[Sequence[PencilArray]],
                           staging_out=None, stages=SIM_STAGES,
                           staging_in=None, scale=None, keep=None,
                           fill="zero") -> None:
    """Every rank's join transpose ``dests[r][c] <- srcs_per_rank[r][c]``
    (:class:`JoinTransposition`): the ordinary n-field pack, one slice copy
    per peer pair, and an unpack that writes the vector-valued destination
    from the ``n`` component slots of every recv block.  ``staging_out``,
    ``stages`` and ``staging_in`` as in :func:`run_transpose_sim_split`.
    ``scale``: the local copy and the unpack multiply; the buffers hold
    unscaled scalars, byte for byte those of the run without a scale.
    ``keep`` / ``fill``: as in :func:`run_transpose_sim_split`."""
    _run_sim_soa(False, dests, srcs_per_rank, staging_out, stages,
                 staging_in, scale, keep, fill)
