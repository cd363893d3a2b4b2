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

from typing import Sequence

import numpy as np

from .array import PencilArray
from .copyexec import apply_copy, apply_copy_conv, apply_fill
from .pencil import Pencil
from .plan import (TransposePlan, build_plan, buffer_nelem_many,
                   copydesc_many, peer_message, stage_descs)
from .plan import fourier_keep  # noqa: F401  (the keep-set helper, re-exported)
from .wire import narrow, resolve_wire, widen

MPI_TAG = 42  # Transpositions.jl:469


def _wire(buf: np.ndarray):
    """A staging-buffer slice as a torch tensor for isend/irecv; opaque
    (void) elements travel as their bytes."""
    import torch
    if buf.dtype.kind == "V":
        buf = buf.view(np.uint8)
    return torch.from_numpy(buf)


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


def _wire_convs(pair):
    """(narrow, widen, round) of a wire pair as elementwise functions."""
    return (lambda x: narrow(x, pair), lambda w: widen(w, pair),
            lambda x: widen(narrow(x, pair), pair))


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
                 fill="zero"):
        """``Transposition(Ao, Ai; method)`` (Transpositions.jl:94-119).

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
        self.method = method
        self.wire = _wire_pair(dest, src, wire_dtype)
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
        if self.wire is not None:
            return self._execute_numpy_wire(use_dist)
        if self.plan.keep is not None:
            return self._execute_numpy_keep(use_dist)
        plan = self.plan
        # vector-valued elements: one opaque B-byte item per element, so the
        # element-unit descriptors apply unchanged
        src_flat = self.src.element_view()
        dst_flat = self.dest.element_view()

        if plan.r_dim is None or plan.nproc_sub == 1:
            if plan.local is not None:
                apply_copy(plan.local, src_flat, dst_flat)
            elif plan.self_pack is not None:
                # in-place: stage through recv buffer (Transpositions.jl:250-264)
                recv_buf = np.empty(plan.recv_nelem_total, dtype=src_flat.dtype)
                apply_copy(plan.self_pack, src_flat, recv_buf)
                apply_copy(plan.self_unpack, recv_buf, dst_flat)
            return

        if not use_dist:
            raise RuntimeError(
                "distributed transpose requires torch.distributed to be "
                "initialised (or use run_transpose_sim for in-process tests)")

        import torch
        import torch.distributed as dist

        # one process per rank: dist rank/world must match the topology
        # (a mismatch would silently address the wrong peers)
        topo = plan.Pi.topology
        if dist.get_world_size() != topo.nranks:
            raise RuntimeError(
                f"torch.distributed world size {dist.get_world_size()} != "
                f"topology nranks {topo.nranks}")
        if dist.get_rank() != plan.rank:
            raise RuntimeError(
                f"torch.distributed rank {dist.get_rank()} != topology "
                f"rank {plan.rank}")

        send_buf = np.empty(plan.send_nelem_total, dtype=src_flat.dtype)
        recv_buf = np.empty(plan.recv_nelem_total, dtype=src_flat.dtype)

        # 1. pack all remote blocks (Transpositions.jl:346-431); in aliased
        # mode also stage the self block into the recv tail BEFORE any write
        # of dst (:394-404)
        for blk in plan.peers:
            if blk.pack is not None:
                apply_copy(blk.pack, src_flat, send_buf)
        if plan.self_pack is not None:
            apply_copy(plan.self_pack, src_flat, recv_buf)

        # 2. exchange: per-peer nonblocking send/recv (:463-479)
        reqs = []
        for blk in plan.peers:
            if blk.peer_k == plan.my_k:
                continue
            if blk.recv_nelem > 0:
                rt = _wire(
                    recv_buf[blk.recv_offset:blk.recv_offset + blk.recv_nelem])
                reqs.append(dist.irecv(rt, src=blk.global_rank, tag=MPI_TAG))
            if blk.send_nelem > 0:
                st = _wire(
                    send_buf[blk.send_offset:blk.send_offset + blk.send_nelem])
                reqs.append(dist.isend(st, dst=blk.global_rank, tag=MPI_TAG))

        # 3. fused local (self) block overlaps the exchange (:394-404 + :530)
        if plan.local is not None:
            apply_copy(plan.local, src_flat, dst_flat)
        elif plan.self_unpack is not None:
            apply_copy(plan.self_unpack, recv_buf, dst_flat)

        for r in reqs:
            r.wait()

        # 4. unpack received blocks (:489-536)
        for blk in plan.peers:
            if blk.unpack is not None:
                apply_copy(blk.unpack, recv_buf, dst_flat)

    def _execute_numpy_keep(self, use_dist: bool):
        """The same stages on a keep plan: one copy per sub-box, messages of
        the kept elements only, and the zero fill next to the local copy."""
        plan = self.plan
        src_flat = self.src.element_view()
        dst_flat = self.dest.element_view()
        send_buf = np.empty(plan.send_nelem_total, dtype=src_flat.dtype)
        recv_buf = np.empty(plan.recv_nelem_total, dtype=src_flat.dtype)

        # every pack (and staged self pack) before any write of dst
        for which, d in stage_descs(plan, 1, 0, 0):
            apply_copy(d, src_flat, send_buf if which == 1 else recv_buf)

        reqs = []
        msgs = [blk for blk in plan.peers if blk.peer_k != plan.my_k
                and (blk.send_nelem or blk.recv_nelem)]
        if msgs:
            if not use_dist:
                raise RuntimeError(
                    "distributed transpose requires torch.distributed to be "
                    "initialised (or use run_transpose_sim for in-process "
                    "tests)")
            import torch.distributed as dist
            topo = plan.Pi.topology
            if dist.get_world_size() != topo.nranks:
                raise RuntimeError(
                    f"torch.distributed world size {dist.get_world_size()} "
                    f"!= topology nranks {topo.nranks}")
            if dist.get_rank() != plan.rank:
                raise RuntimeError(
                    f"torch.distributed rank {dist.get_rank()} != topology "
                    f"rank {plan.rank}")
            # a peer with nothing kept is absent from the exchange
            for blk in msgs:
                if blk.recv_nelem > 0:
                    rt = _wire(recv_buf[
                        blk.recv_offset:blk.recv_offset + blk.recv_nelem])
                    reqs.append(dist.irecv(rt, src=blk.global_rank,
                                           tag=MPI_TAG))
                if blk.send_nelem > 0:
                    st = _wire(send_buf[
                        blk.send_offset:blk.send_offset + blk.send_nelem])
                    reqs.append(dist.isend(st, dst=blk.global_rank,
                                           tag=MPI_TAG))

        for which, d in stage_descs(plan, 1, 0, 1):
            apply_copy(d, src_flat if which == 0 else recv_buf, dst_flat)
        for fd in plan.fills:
            apply_fill(fd, dst_flat)
        for r in reqs:
            r.wait()
        for _, d in stage_descs(plan, 1, 0, 2):
            apply_copy(d, recv_buf, dst_flat)

    def _execute_numpy_wire(self, use_dist: bool):
        """The same stages with a reduced-precision wire: staging buffers of
        the wire type, packs narrow, unpacks widen, the local copy rounds."""
        plan, pair = self.plan, self.wire
        nc = self.src.ncomp * pair.comps  # stored scalars per element
        src = self.src.data.view(pair.stored)
        dst = self.dest.data.view(pair.stored)
        nar, wid, rnd = _wire_convs(pair)
        send_buf = np.empty(plan.send_nelem_total * nc, dtype=pair.carrier)
        recv_buf = np.empty(plan.recv_nelem_total * nc, dtype=pair.carrier)
        exchanging = plan.r_dim is not None and plan.nproc_sub > 1

        for blk in plan.peers:
            if blk.pack is not None:
                apply_copy_conv(blk.pack, src, send_buf, nc, nar)
        if plan.self_pack is not None:
            apply_copy_conv(plan.self_pack, src, recv_buf, nc, nar)

        reqs = []
        if exchanging:
            if not use_dist:
                raise RuntimeError(
                    "distributed transpose requires torch.distributed to be "
                    "initialised (or use run_transpose_sim for in-process "
                    "tests)")
            import torch
            import torch.distributed as dist
            topo = plan.Pi.topology
            if dist.get_world_size() != topo.nranks:
                raise RuntimeError(
                    f"torch.distributed world size {dist.get_world_size()} "
                    f"!= topology nranks {topo.nranks}")
            if dist.get_rank() != plan.rank:
                raise RuntimeError(
                    f"torch.distributed rank {dist.get_rank()} != topology "
                    f"rank {plan.rank}")
            for blk in plan.peers:
                if blk.peer_k == plan.my_k:
                    continue
                # the wire-typed slices travel as their bytes
                if blk.recv_nelem > 0:
                    rt = torch.from_numpy(recv_buf[
                        blk.recv_offset * nc:
                        (blk.recv_offset + blk.recv_nelem) * nc
                    ].view(np.uint8))
                    reqs.append(dist.irecv(rt, src=blk.global_rank,
                                           tag=MPI_TAG))
                if blk.send_nelem > 0:
                    st = torch.from_numpy(send_buf[
                        blk.send_offset * nc:
                        (blk.send_offset + blk.send_nelem) * nc
                    ].view(np.uint8))
                    reqs.append(dist.isend(st, dst=blk.global_rank,
                                           tag=MPI_TAG))

        if plan.local is not None:
            apply_copy_conv(plan.local, src, dst, nc, rnd)
        elif plan.self_unpack is not None:
            apply_copy_conv(plan.self_unpack, recv_buf, dst, nc, wid)
        for r in reqs:
            r.wait()
        for blk in plan.peers:
            if blk.unpack is not None:
                apply_copy_conv(blk.unpack, recv_buf, dst, nc, wid)

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
                   fill="zero") -> PencilArray:
    """``transpose!(dest, src; method)`` (Transpositions.jl:161-169)."""
    if dest is src:
        return dest
    return Transposition(dest, src, method=method, wire_dtype=wire_dtype,
                         keep=keep, fill=fill).execute()


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
    :class:`Transposition`.  ``keep`` / ``fill``: a truncated transpose of
    every field, as in :class:`Transposition`."""

    def __init__(self, dests: Sequence[PencilArray],
                 srcs: Sequence[PencilArray], wire_dtype=None, keep=None,
                 fill="zero"):
        _check_keep_wire(keep, wire_dtype)
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
        self.keep, self.fill = keep, fill
        self.wire = _wire_pair(d0, s0, wire_dtype)
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
                          fill=self.fill).execute()

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
                        keep=None, fill="zero"):
    """``transpose!`` of every pair ``dests[i] <- srcs[i]`` in one call."""
    return MultiTransposition(dests, srcs, wire_dtype=wire_dtype, keep=keep,
                              fill=fill).execute()


# ----------------------------------------------------------------------
# In-process multi-rank simulation (test harness only): runs every rank's
# pack/exchange/unpack inside one process, memcpy standing in for the
# exchange.  This is how CPU tests cover P>1 without spawning processes.
# ----------------------------------------------------------------------

def run_transpose_sim(dests: Sequence[PencilArray],
                      srcs: Sequence[PencilArray],
                      staging_out=None, wire_dtype=None, keep=None,
                      fill="zero") -> None:
    """``staging_out``, if a dict, receives the final ``send``/``recv``
    staging buffers per rank.  ``wire_dtype``: a reduced-precision wire (see
    :class:`Transposition`); the staging buffers then hold wire scalars.
    ``keep`` / ``fill``: a truncated transpose (see :class:`Transposition`);
    the staging buffers then hold the kept elements only."""
    _check_keep_wire(keep, wire_dtype)
    if wire_dtype is not None or keep is not None:
        return run_transpose_sim_many([[d] for d in dests],
                                      [[s] for s in srcs], staging_out,
                                      wire_dtype=wire_dtype, keep=keep,
                                      fill=fill)
    nranks = len(srcs)
    plans = [build_plan(s.pencil, d.pencil, r, s.extra_dims,
                        aliased=_arrays_alias(s.data, d.data))
             for r, (d, s) in enumerate(zip(dests, srcs))]
    for d, s in zip(dests, srcs):
        if d.elem_dims != s.elem_dims:
            raise ValueError(
                f"incompatible element dimensions of PencilArrays: "
                f"{s.elem_dims} != {d.elem_dims}")
    sflat = [s.element_view() for s in srcs]
    dflat = [d.element_view() for d in dests]

    send_bufs = [np.empty(p.send_nelem_total, dtype=sflat[r].dtype)
                 for r, p in enumerate(plans)]
    recv_bufs = [np.empty(p.recv_nelem_total, dtype=sflat[r].dtype)
                 for r, p in enumerate(plans)]

    # pack on every rank (incl. staged self blocks, before any dst write)
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.pack is not None:
                apply_copy(blk.pack, sflat[r], send_bufs[r])
        if p.self_pack is not None:
            apply_copy(p.self_pack, sflat[r], recv_bufs[r])
    for r, p in enumerate(plans):
        if p.local is not None:
            apply_copy(p.local, sflat[r], dflat[r])
        elif p.self_unpack is not None:
            apply_copy(p.self_unpack, recv_bufs[r], dflat[r])

    # exchange: copy each send block into the receiver's recv buffer
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.peer_k == p.my_k or blk.send_nelem == 0:
                continue
            # The matching recv block on the peer: the peer's PeerBlock whose
            # peer coordinate equals MY coordinate along R.
            q = plans[blk.global_rank]
            rblk = q.peers[p.my_k]
            assert rblk.global_rank == r and rblk.recv_nelem == blk.send_nelem, \
                (r, blk, rblk)
            recv_bufs[blk.global_rank][
                rblk.recv_offset:rblk.recv_offset + rblk.recv_nelem] = \
                send_bufs[r][blk.send_offset:blk.send_offset + blk.send_nelem]

    # unpack on every rank
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.unpack is not None:
                apply_copy(blk.unpack, recv_bufs[r], dflat[r])
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs


def run_transpose_sim_many(dests_per_rank: Sequence[Sequence[PencilArray]],
                           srcs_per_rank: Sequence[Sequence[PencilArray]],
                           staging_out=None, wire_dtype=None, keep=None,
                           fill="zero") -> None:
    """:func:`run_transpose_sim` for ``n`` fields per rank with the
    multi-field staging layout (plan.py): every field of a rank is packed
    into ONE n-fold send buffer, and the exchange is ONE slice copy per peer
    pair of ``n * c`` elements — the "one message per peer" contract.
    ``dests_per_rank[r][f]`` / ``srcs_per_rank[r][f]`` is field ``f`` on
    rank ``r``.  ``staging_out``, if a dict, receives the final
    ``send``/``recv`` buffers per rank (tests compare them).
    ``wire_dtype``: a reduced-precision wire; the staging buffers then hold
    wire scalars (bfloat16 as uint16 patterns), packs narrow, unpacks widen
    and the local copy rounds.  ``keep`` / ``fill``: a truncated transpose
    through the sub-box tables of the keep plan."""
    _check_keep_wire(keep, wire_dtype)
    if wire_dtype is not None:
        return _run_sim_many_wire(dests_per_rank, srcs_per_rank, staging_out,
                                  wire_dtype)
    if keep is not None:
        return _run_sim_many_keep(dests_per_rank, srcs_per_rank, staging_out,
                                  keep, fill)
    nranks = len(srcs_per_rank)
    n = len(srcs_per_rank[0])
    if n < 1 or any(len(x) != n for x in srcs_per_rank) or \
            any(len(x) != n for x in dests_per_rank):
        raise ValueError("every rank needs the same number (>= 1) of fields")
    plans = []
    for r in range(nranks):
        s0, d0 = srcs_per_rank[r][0], dests_per_rank[r][0]
        aliased = any(_arrays_alias(s.data, d.data)
                      for s in srcs_per_rank[r] for d in dests_per_rank[r])
        plans.append(build_plan(s0.pencil, d0.pencil, r, s0.extra_dims,
                                aliased=aliased))
    sflat = [[s.element_view() for s in row] for row in srcs_per_rank]
    dflat = [[d.element_view() for d in row] for row in dests_per_rank]
    dt = sflat[0][0].dtype
    send_bufs, recv_bufs = [], []
    for p in plans:
        ns, nr = buffer_nelem_many(p, n)
        send_bufs.append(np.empty(ns, dtype=dt))
        recv_bufs.append(np.empty(nr, dtype=dt))

    # pack every field on every rank (incl. staged self blocks) before any
    # destination is written
    for r, p in enumerate(plans):
        for f in range(n):
            for blk in p.peers:
                if blk.pack is not None:
                    apply_copy(copydesc_many(p, n, f, 1, blk.peer_k),
                               sflat[r][f], send_bufs[r])
            if p.self_pack is not None:
                apply_copy(copydesc_many(p, n, f, 3), sflat[r][f],
                           recv_bufs[r])
    for r, p in enumerate(plans):
        for f in range(n):
            if p.local is not None:
                apply_copy(p.local, sflat[r][f], dflat[r][f])
            elif p.self_unpack is not None:
                apply_copy(copydesc_many(p, n, f, 4), recv_bufs[r],
                           dflat[r][f])

    # exchange: ONE slice copy per peer pair, all n fields in it
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
            recv_bufs[blk.global_rank][ro:ro + rn] = send_bufs[r][so:so + sn]

    # unpack every field on every rank
    for r, p in enumerate(plans):
        for f in range(n):
            for blk in p.peers:
                if blk.unpack is not None:
                    apply_copy(copydesc_many(p, n, f, 2, blk.peer_k),
                               recv_bufs[r], dflat[r][f])
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs


def _run_sim_many_keep(dests_per_rank, srcs_per_rank, staging_out, keep,
                       fill) -> None:
    """run_transpose_sim_many on keep plans: the same stages over the
    sub-box tables, one slice copy of the KEPT elements per peer pair (none
    for a peer with nothing kept), and the zero fill of every field."""
    nranks = len(srcs_per_rank)
    n = len(srcs_per_rank[0])
    if n < 1 or any(len(x) != n for x in srcs_per_rank) or \
            any(len(x) != n for x in dests_per_rank):
        raise ValueError("every rank needs the same number (>= 1) of fields")
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
    sflat = [[s.element_view() for s in row] for row in srcs_per_rank]
    dflat = [[d.element_view() for d in row] for row in dests_per_rank]
    dt = sflat[0][0].dtype
    send_bufs, recv_bufs = [], []
    for p in plans:
        ns, nr = buffer_nelem_many(p, n)
        send_bufs.append(np.empty(ns, dtype=dt))
        recv_bufs.append(np.empty(nr, dtype=dt))

    for r, p in enumerate(plans):
        for f in range(n):
            for which, d in stage_descs(p, n, f, 0):
                apply_copy(d, sflat[r][f],
                           send_bufs[r] if which == 1 else recv_bufs[r])
    for r, p in enumerate(plans):
        for f in range(n):
            for which, d in stage_descs(p, n, f, 1):
                apply_copy(d, sflat[r][f] if which == 0 else recv_bufs[r],
                           dflat[r][f])
            for fd in p.fills:
                apply_fill(fd, dflat[r][f])

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
            recv_bufs[blk.global_rank][ro:ro + rn] = send_bufs[r][so:so + sn]

    for r, p in enumerate(plans):
        for f in range(n):
            for _, d in stage_descs(p, n, f, 2):
                apply_copy(d, recv_bufs[r], dflat[r][f])
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs


def _run_sim_many_wire(dests_per_rank, srcs_per_rank, staging_out,
                       wire_dtype) -> None:
    """run_transpose_sim_many with a reduced-precision wire: the same
    staging layout in elements, every buffer in wire scalars."""
    nranks = len(srcs_per_rank)
    n = len(srcs_per_rank[0])
    if n < 1 or any(len(x) != n for x in srcs_per_rank) or \
            any(len(x) != n for x in dests_per_rank):
        raise ValueError("every rank needs the same number (>= 1) of fields")
    s00 = next(s for row in srcs_per_rank for s in row)
    pair = _wire_pair(dests_per_rank[0][0], s00, wire_dtype)
    nc = s00.ncomp * pair.comps
    nar, wid, rnd = _wire_convs(pair)
    plans = []
    for r in range(nranks):
        s0, d0 = srcs_per_rank[r][0], dests_per_rank[r][0]
        aliased = any(_arrays_alias(s.data, d.data)
                      for s in srcs_per_rank[r] for d in dests_per_rank[r])
        plans.append(build_plan(s0.pencil, d0.pencil, r, s0.extra_dims,
                                aliased=aliased))
    sflat = [[s.data.view(pair.stored) for s in row] for row in srcs_per_rank]
    dflat = [[d.data.view(pair.stored) for d in row]
             for row in dests_per_rank]
    send_bufs, recv_bufs = [], []
    for p in plans:
        ns, nr = buffer_nelem_many(p, n)
        send_bufs.append(np.empty(ns * nc, dtype=pair.carrier))
        recv_bufs.append(np.empty(nr * nc, dtype=pair.carrier))

    for r, p in enumerate(plans):
        for f in range(n):
            for blk in p.peers:
                if blk.pack is not None:
                    apply_copy_conv(copydesc_many(p, n, f, 1, blk.peer_k),
                                    sflat[r][f], send_bufs[r], nc, nar)
            if p.self_pack is not None:
                apply_copy_conv(copydesc_many(p, n, f, 3), sflat[r][f],
                                recv_bufs[r], nc, nar)
    for r, p in enumerate(plans):
        for f in range(n):
            if p.local is not None:
                apply_copy_conv(p.local, sflat[r][f], dflat[r][f], nc, rnd)
            elif p.self_unpack is not None:
                apply_copy_conv(copydesc_many(p, n, f, 4), recv_bufs[r],
                                dflat[r][f], nc, wid)

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
            recv_bufs[blk.global_rank][ro * nc:(ro + rn) * nc] = \
                send_bufs[r][so * nc:(so + sn) * nc]

    for r, p in enumerate(plans):
        for f in range(n):
            for blk in p.peers:
                if blk.unpack is not None:
                    apply_copy_conv(copydesc_many(p, n, f, 2, blk.peer_k),
                                    recv_bufs[r], dflat[r][f], nc, wid)
    if staging_out is not None:
        staging_out["send"] = send_bufs
        staging_out["recv"] = recv_bufs
