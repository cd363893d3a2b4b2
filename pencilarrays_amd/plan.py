"""Transposition plan: the block tables of the global pencil transpose.

Restates the control path of src/Transpositions/Transpositions.jl as pure
metadata.  For a given rank, input pencil Pi and output pencil Po (with the
decompositions differing along one topology dimension R, Transpositions.jl:111)
this computes exactly which sub-blocks are packed/sent/received/unpacked and
with which layout:

- peer enumeration = ``get_remote_indices`` (:542-552): coordinates equal to
  mine except along R, k = 0..P-1; subgroup rank of peer k is k
  (MPITopologies.jl:229-242).
- send block to peer k = intersect(Pi.axes_local, Po.axes_all[k])   (:383)
- recv block from peer k = intersect(Po.axes_local, Pi.axes_all[k]) (:388,:521)
- the self block (k == my coord along R) is placed at the END of the receive
  buffer (:394-404); other blocks at offsets accumulated in k order (:414-415).
- pack order inside a block: column-major (first memory axis fastest) over the
  block's extents in Pi *memory* order, extra dims outermost (copy_range!,
  :554-586).
- unpack: the received block, reshaped column-major to its extents gathered by
  permutation(Pi) (:527, :599-600), is scattered into the Po parent window at
  ``perm * o_range_iperm`` with ``perm = permutation(Po)/permutation(Pi)``
  (:506, :602).

Every data movement is expressed as a :class:`CopyDesc` — an N-d strided copy
``dst[Σ j_i·dstride_i] = src[Σ j_i·sstride_i]`` over ``dims`` — which is what
the HIP copy engine, the numpy executor and the C++ engine all execute.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

from .pencil import (
    Pencil,
    Region,
    range_intersect,
    region_intersect,
    region_lengths,
    region_nelem,
)
from .permutations import perm_apply, perm_inv, perm_relative

# --------------------------------------------------------------------------


@dataclass(frozen=True)
class CopyDesc:
    """dst[doffset + Σ j_i·dstrides_i] = src[soffset + Σ j_i·sstrides_i],
    j over ``dims`` (all in elements)."""
    dims: Tuple[int, ...]
    sstrides: Tuple[int, ...]
    soffset: int
    dstrides: Tuple[int, ...]
    doffset: int

    @property
    def nelem(self) -> int:
        return math.prod(self.dims) if self.dims else 1


def _colmajor_strides(dims: Tuple[int, ...]) -> Tuple[int, ...]:
    st, acc = [], 1
    for d in dims:
        st.append(acc)
        acc *= d
    return tuple(st)


def normalize_desc(d: CopyDesc) -> CopyDesc:
    """Drop unit axes, sort by ascending src stride, merge adjacent axes that
    are contiguous on BOTH sides.  Semantics-preserving relabeling."""
    axes = [(dim, ss, ds) for dim, ss, ds in
            zip(d.dims, d.sstrides, d.dstrides) if dim != 1]
    if not axes:
        return CopyDesc((1,), (1,), d.soffset, (1,), d.doffset)
    axes.sort(key=lambda a: a[1])
    merged = [axes[0]]
    for dim, ss, ds in axes[1:]:
        pdim, pss, pds = merged[-1]
        if ss == pss * pdim and ds == pds * pdim:
            merged[-1] = (pdim * dim, pss, pds)
        else:
            merged.append((dim, ss, ds))
    dims, ss, ds = zip(*merged)
    return CopyDesc(dims, ss, d.soffset, ds, d.doffset)


# --------------------------------------------------------------------------


def _single(subs, keep):
    """Read-only single-descriptor view of a sub-block list: the one
    descriptor of an ordinary plan; None on a keep plan or when absent."""
    if keep is not None or not subs:
        return None
    return getattr(subs[0], "desc", subs[0])


@dataclass
class PeerBlock:
    peer_k: int                 # coordinate along R == subgroup rank
    global_rank: int            # rank in the full topology
    send_region: Region         # global logical ranges I send to this peer
    recv_region: Region         # global logical ranges I receive from it
    send_nelem: int
    recv_nelem: int
    send_offset: int            # element offset into send staging buffer
    recv_offset: int            # element offset into recv staging buffer
    keep: Optional[Tuple[Tuple[int, int], ...]] = None  # the plan's keep set
    # one staging block per non-empty sub-box of the block: src parent ->
    # send buffer, recv buffer -> dst parent (empty for the self block).  An
    # ordinary plan, whose keep set is everything, has at most one each.
    pack_subs: List["SubBlock"] = field(default_factory=list)
    unpack_subs: List["SubBlock"] = field(default_factory=list)

    pack = property(lambda self: _single(self.pack_subs, self.keep))
    unpack = property(lambda self: _single(self.unpack_subs, self.keep))


@dataclass
class TransposePlan:
    rank: int
    Pi: Pencil
    Po: Pencil
    extra_dims: Tuple[int, ...]
    r_dim: Optional[int]            # R; None = same decomposition (local path)
    nproc_sub: int                  # subgroup size P (1 if local path)
    my_k: int                       # my coordinate along R
    peers: List[PeerBlock] = field(default_factory=list)
    send_nelem_total: int = 0
    recv_nelem_total: int = 0       # staging incl. self tail when aliased
    aliased: bool = False
    # truncated transposes (keep plans): the keep set as (a, b) per logical
    # dim and the fill mode; every count and offset is then in KEPT elements
    keep: Optional[Tuple[Tuple[int, int], ...]] = None
    fill: int = 0
    # The self block, one entry per non-empty sub-box (at most one on an
    # ordinary plan): fused src-window -> dst-window copies, or in aliased
    # (in-place) mode staged through the recv-buffer tail (the reference's
    # aliasing path: Transpositions.jl:250-264 for the local case, :394-404
    # placement for the distributed case), so every read of src completes
    # before any write of dst.
    local_subs: List[CopyDesc] = field(default_factory=list)
    self_pack_subs: List["SubBlock"] = field(default_factory=list)
    self_unpack_subs: List["SubBlock"] = field(default_factory=list)
    fills: List["FillDesc"] = field(default_factory=list)

    local = property(lambda self: _single(self.local_subs, self.keep))
    self_pack = property(lambda self: _single(self.self_pack_subs, self.keep))
    self_unpack = property(
        lambda self: _single(self.self_unpack_subs, self.keep))

    @property
    def subgroup_global_ranks(self) -> List[int]:
        if self.r_dim is None:
            return [self.rank]
        return self.Pi.topology.subgroup_ranks(self.rank, self.r_dim)


def _parent_strides(p: Pencil, rank: int,
                    extra_dims: Tuple[int, ...]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(mem_dims, strides) of the local parent array: memory-order local dims
    plus extra dims appended, column-major (axis 0 fastest) — byte-identical
    to the reference's Julia parent (arrays.jl:134-138)."""
    mem = tuple(p.size_local(rank, memory_order=True)) + tuple(extra_dims)
    return mem, _colmajor_strides(mem)


def _window_desc_src(p: Pencil, rank: int, region: Region,
                     extra_dims: Tuple[int, ...]) -> Tuple[Tuple[int, ...], Tuple[int, ...], int]:
    """dims/strides/offset of a global ``region`` as a window of the local
    parent of pencil ``p``, axes in p's memory order (+ extra axes)."""
    local = p.to_local(rank, region, memory_order=True)  # mem-order local ranges
    _, pst = _parent_strides(p, rank, extra_dims)
    dims = tuple(hi - lo for lo, hi in local) + tuple(extra_dims)
    offset = sum(lo * pst[i] for i, (lo, _) in enumerate(local))
    return dims, pst, offset  # one stride per mem axis, then the extra axes


def build_plan(Pi: Pencil, Po: Pencil, rank: int,
               extra_dims: Tuple[int, ...] = (),
               aliased: bool = False, keep=None,
               fill="zero") -> TransposePlan:
    """The block tables of ``rank``'s transpose ``Pi -> Po``.

    ``keep`` (a sequence of ``(a, b)`` per logical dim, ``None`` entries
    meaning full) builds a truncated transpose: every block is intersected
    with the keep set, every count and offset is in KEPT elements, each block
    holds one descriptor per non-empty sub-box, and ``fills`` lists the
    destination windows outside the keep set when ``fill`` is zero.  Without
    it the keep set is everything: a block is its own single sub-box,
    readable as ``pack`` / ``unpack`` / ``local`` / ``self_pack`` /
    ``self_unpack``, and ``fill`` is ignored."""
    extra_dims = tuple(int(e) for e in extra_dims)
    R = Pi.transpose_dim(Po)  # validates compatibility
    n, E = Pi.ndims, len(extra_dims)
    size = Pi.size_global
    pex = math.prod(extra_dims or (1,))
    fcode = FILL_NONE
    if keep is not None:
        keep = normalize_keep(size, keep)
        fcode = fill_code(fill)

    # Relative permutation Po-mem-axis -> Pi-mem-axis (Transpositions.jl:506):
    # dest memory axis i' holds logical dim permo[i'], which sits at source
    # memory axis inv(permi)[permo[i']].
    q_rel = perm_relative(Po.perm, Pi.perm)
    q_full = tuple(q_rel) + tuple(n + i for i in range(E))
    inv_q = perm_inv(q_full)
    _, pst_o = _parent_strides(Po, rank, extra_dims)

    plan = TransposePlan(
        rank=rank, Pi=Pi, Po=Po, extra_dims=extra_dims, r_dim=R,
        nproc_sub=1 if R is None else Pi.topology.dims[R], my_k=0,
        aliased=aliased, keep=keep, fill=fcode)

    def boxes(region: Region) -> List[Region]:
        """The sub-boxes of a block.  An ordinary plan keeps everything, so
        the region itself, gated as ordinary plans always were: a block of a
        subgroup on its element count, extras included, and the
        same-decomposition block on its geometry alone."""
        if keep is not None:
            return sub_boxes(region, keep, size)
        nelem = region_nelem(region) * (1 if R is None else pex)
        return [region] if nelem > 0 else []

    def to_dst(buf_dims, box: Region, src_strides, src_offset) -> CopyDesc:
        """CopyDesc moving a block laid out on ``src`` (axes = Pi-mem order +
        extras, strides given) into the Po parent window of ``box``: buffer
        axis j feeds dest mem axis inv_q[j]."""
        starts = tuple(lo for lo, _ in
                       Po.to_local(rank, box, memory_order=True)) + (0,) * E
        dstrides = tuple(pst_o[inv_q[j]] for j in range(n + E))
        doffset = sum(starts[i] * pst_o[i] for i in range(n + E))
        return normalize_desc(CopyDesc(buf_dims, src_strides, src_offset,
                                       dstrides, doffset))

    def pack_sub(box: Region, off: int) -> SubBlock:
        sdims, sst, soff = _window_desc_src(Pi, rank, box, extra_dims)
        return SubBlock(box, off, region_nelem(box) * pex, normalize_desc(
            CopyDesc(sdims, sst, soff, _colmajor_strides(sdims), off)))

    def unpack_sub(box: Region, off: int) -> SubBlock:
        # the buffer holds the box in Pi memory order of ITS window
        bdims = perm_apply(Pi.perm, region_lengths(box)) + extra_dims
        return SubBlock(box, off, region_nelem(box) * pex,
                        to_dst(bdims, box, _colmajor_strides(bdims), off))

    def self_block(region: Region, off: int) -> int:
        """The self block: the fused direct src-window -> dst-window permuted
        copy (replaces the reference's copy to the recv_buf tail :394-404
        followed by copy_permuted! — same values, half the HBM traffic).  In
        aliased (in-place) mode that copy would read windows the unpacks
        overwrite, so the block is staged at ``off`` like the reference.
        Returns the end offset."""
        for box in boxes(region):
            if aliased:
                ps = pack_sub(box, off)
                plan.self_pack_subs.append(ps)
                plan.self_unpack_subs.append(unpack_sub(box, off))
                off += ps.nelem
            else:
                sdims, sst, soff = _window_desc_src(Pi, rank, box, extra_dims)
                plan.local_subs.append(to_dst(sdims, box, sst, soff))
        return off

    if fcode == FILL_ZERO:
        axes_o = Po.axes_for_rank(rank)
        for box in fill_regions(keep, size):
            box = region_intersect(box, axes_o)
            if region_nelem(box) == 0 or pex == 0:
                continue
            loc = Po.to_local(rank, box, memory_order=True)
            dims = tuple(hi - lo for lo, hi in loc) + extra_dims
            off = sum(lo * pst_o[i] for i, (lo, _) in enumerate(loc))
            plan.fills.append(_fill_desc(dims, pst_o, off))

    if R is None:
        # Same decomposition: plain copy or local permutation
        # (transpose_impl!(::Nothing), Transpositions.jl:214-271; in-place
        # variant stages through recv_buf, :250-264).
        plan.recv_nelem_total = self_block(Pi.axes_for_rank(rank), 0)
        return plan

    topo = Pi.topology
    coords = topo.cart_coords(rank)
    plan.my_k = coords[R]
    axes_local_i = Pi.axes_for_rank(rank)
    axes_local_o = Po.axes_for_rank(rank)
    isend = irecv = 0
    for k in range(topo.dims[R]):
        pc = list(coords)
        pc[R] = k
        pc = tuple(pc)
        srange = region_intersect(axes_local_i, Po.axes_for_coords(pc))
        rrange = region_intersect(axes_local_o, Pi.axes_for_coords(pc))
        sboxes, rboxes = boxes(srange), boxes(rrange)
        blk = PeerBlock(
            peer_k=k, global_rank=topo.cart_rank(pc), send_region=srange,
            recv_region=rrange,
            send_nelem=sum(region_nelem(b) for b in sboxes) * pex,
            recv_nelem=sum(region_nelem(b) for b in rboxes) * pex,
            send_offset=0, recv_offset=0, keep=keep)
        if k != plan.my_k:
            blk.send_offset, blk.recv_offset = isend, irecv
            for box in sboxes:
                blk.pack_subs.append(pack_sub(box, isend))
                isend += blk.pack_subs[-1].nelem
            for box in rboxes:
                blk.unpack_subs.append(unpack_sub(box, irecv))
                irecv += blk.unpack_subs[-1].nelem
        plan.peers.append(blk)
    plan.send_nelem_total = isend
    self_blk = plan.peers[plan.my_k]
    self_blk.recv_offset = irecv  # the self block sits at the recv tail
    plan.recv_nelem_total = self_block(self_blk.send_region, irecv)
    return plan


# --------------------------------------------------------------------------
# Truncated transposes: move only a kept product set of indices.
#
# A keep set is K = K_0 x ... x K_{N-1} over the logical dims with
# K_d = [0, a_d) U [N_d - b_d, N_d): the low and the high wavenumbers of a
# c2c dimension, or b = 0 for an r2c one.  Every block of the ordinary plan
# (a peer's send region, a peer's recv region, the self block) is intersected
# with K, which leaves up to 2^N sub-boxes; each non-empty sub-box is a
# staging block of its own with an ordinary normalised CopyDesc.  Sender and
# receiver derive the same sub-boxes from the same ranges, in the same order.
# The reference has no such option (transpose! moves every element).
# --------------------------------------------------------------------------

FILL_NONE, FILL_ZERO = 0, 1


@dataclass(frozen=True)
class SubBlock:
    """One sub-box of a block: its global region, its staging block
    (``offset``, ``nelem`` in elements) and its descriptor."""
    region: Region
    offset: int
    nelem: int
    desc: CopyDesc


@dataclass(frozen=True)
class FillDesc:
    """A destination-only window of the output parent:
    ``dst[doffset + sum j_i * dstrides_i] = 0`` for j over ``dims``."""
    dims: Tuple[int, ...]
    dstrides: Tuple[int, ...]
    doffset: int

    @property
    def nelem(self) -> int:
        return math.prod(self.dims) if self.dims else 1


def fill_code(fill) -> int:
    """``"zero"``/1 -> FILL_ZERO, ``None``/``"none"``/0 -> FILL_NONE."""
    if fill is None or fill == "none":
        return FILL_NONE
    if fill == "zero":
        return FILL_ZERO
    if isinstance(fill, int) and not isinstance(fill, bool) and \
            fill in (FILL_NONE, FILL_ZERO):
        return fill
    raise ValueError(f"fill must be 'zero' or None/'none' (got {fill!r})")


def normalize_keep(size_global: Sequence[int], keep) -> Tuple[Tuple[int, int], ...]:
    """Validate a keep set against the global size; ``None`` entries mean
    the full range ``(N_d, 0)``."""
    keep = list(keep)
    if len(keep) != len(size_global):
        raise ValueError(
            f"keep needs one (a, b) per logical dim: got {len(keep)} for "
            f"{len(size_global)} dims")
    out = []
    for d, (kd, N) in enumerate(zip(keep, size_global)):
        if kd is None:
            out.append((int(N), 0))
            continue
        a, b = (int(v) for v in kd)
        if a < 0 or b < 0 or a + b > N:
            raise ValueError(
                f"keep[{d}] = ({a}, {b}) must satisfy a, b >= 0 and "
                f"a + b <= {N}")
        out.append((a, b))
    return tuple(out)


def fourier_keep(size_global: Sequence[int], kmax,
                 real_dim: Optional[int] = None):
    """The usual keep set of a pseudo-spectral code: wavenumbers
    ``|k_d| <= kmax_d``.  A c2c dim keeps ``a = kmax_d + 1`` low and
    ``b = kmax_d`` high indices, the r2c dim ``real_dim`` (which stores only
    ``k >= 0``) ``a = kmax_d + 1, b = 0``.  ``kmax`` is one int for every dim
    or a sequence with ``None`` entries for untruncated dims."""
    n = len(size_global)
    if isinstance(kmax, int):
        kmax = [kmax] * n
    kmax = list(kmax)
    if len(kmax) != n:
        raise ValueError("kmax needs one entry per logical dim")
    out = []
    for d in range(n):
        if kmax[d] is None:
            out.append(None)
            continue
        k = int(kmax[d])
        a, b = k + 1, (0 if d == real_dim else k)
        if k < 0 or a + b > size_global[d]:
            raise ValueError(
                f"kmax[{d}] = {k} does not fit dimension {size_global[d]}")
        out.append((a, b))
    return out


def _keep_ranges(a: int, b: int, N: int) -> List[Tuple[int, int]]:
    """The ranges of K_d, low before high; adjacent ranges merge."""
    if a + b >= N:
        return [(0, N)]
    return [(0, a), (N - b, N)]


def _box_product(per_dim: List[List[Tuple[int, int]]]) -> List[Region]:
    """Every combination of one range per dim, dim 0 varying fastest."""
    out: List[Region] = [()]
    for ranges in reversed(per_dim):
        out = [(r,) + tail for tail in out for r in ranges]
    return out


def sub_boxes(region: Region, keep, size_global) -> List[Region]:
    """The non-empty sub-boxes of ``region`` intersected with the keep set,
    low range before high range, dim 0 varying fastest."""
    per_dim = [[range_intersect(rg, kr) for kr in _keep_ranges(a, b, N)]
               for rg, (a, b), N in zip(region, keep, size_global)]
    return [box for box in _box_product(per_dim) if region_nelem(box) > 0]


def fill_regions(keep, size_global) -> List[Region]:
    """The complement of the keep set as disjoint global boxes: for
    d = 0..N-1, (kept in dims < d) x (dropped range [a_d, N_d - b_d) of dim
    d) x (everything in dims > d).  A kept factor with both a low and a high
    range contributes both (low first, dim 0 fastest), so there are at most
    N boxes when every b_d = 0."""
    n = len(size_global)
    out = []
    for d in range(n):
        a, b = keep[d]
        if size_global[d] - b <= a:
            continue
        per_dim = ([_keep_ranges(*keep[j], size_global[j]) for j in range(d)]
                   + [[(a, size_global[d] - b)]]
                   + [[(0, size_global[j])] for j in range(d + 1, n)])
        out.extend(_box_product(per_dim))
    return out


def _fill_desc(dims, strides, offset) -> FillDesc:
    """Drop unit axes and merge contiguous ones (strides ascend already)."""
    axes = [(dim, st) for dim, st in zip(dims, strides) if dim != 1]
    if not axes:
        return FillDesc((1,), (1,), offset)
    merged = [axes[0]]
    for dim, st in axes[1:]:
        pdim, pst = merged[-1]
        if st == pst * pdim:
            merged[-1] = (pdim * dim, pst)
        else:
            merged.append((dim, st))
    dims, st = zip(*merged)
    return FillDesc(tuple(dims), tuple(st), offset)


def build_keep_plan(Pi: Pencil, Po: Pencil, rank: int,
                    extra_dims: Tuple[int, ...], aliased: bool, keep,
                    fill="zero") -> TransposePlan:
    """The plan of a truncated transpose: ``build_plan(..., keep=keep)``."""
    return build_plan(Pi, Po, rank, extra_dims, aliased, keep, fill)


# --------------------------------------------------------------------------
# Multi-field staging layout (n fields of one pencil pair, one plan).
#
# The plan stays per field in element units; the staging buffers are n times
# its sizes.  A staging block that starts at element offset ``o`` with ``c``
# elements in the single-field plan (a peer's send block, a peer's recv
# block, the aliased self block in the recv tail) holds field ``f`` at
# ``n*o + f*c``.  Blocks are consecutive, so this tiles the n-fold buffer
# exactly, and peer k's message is the contiguous range
# ``[n*o_k, n*(o_k + c_k))``: one send and one recv per peer whatever n is.
# ``n = 1`` is the single-field layout.
# --------------------------------------------------------------------------

def many_shift(n: int, f: int, o: int, c: int) -> int:
    """How far field ``f`` of ``n`` moves the staging-side offset of a block
    at offset ``o`` with ``c`` elements: ``n*o + f*c - o``."""
    return (n - 1) * o + f * c


def _check_many(n: int, f: int = 0):
    if n < 1:
        raise ValueError(f"n must be >= 1 (got {n})")
    if not 0 <= f < n:
        raise ValueError(f"field {f} out of range for n = {n}")


def _subs(plan: TransposePlan, which: int, k: int):
    """The sub-block list behind ``which``: 0 local, 1 pack of peer k,
    2 unpack of peer k, 3 staged self pack, 4 staged self unpack.  None for
    a peer the plan does not have."""
    if which == 0:
        return plan.local_subs
    if which in (3, 4):
        return plan.self_pack_subs if which == 3 else plan.self_unpack_subs
    if plan.r_dim is None or not 0 <= k < len(plan.peers):
        return None
    if which == 1:
        return plan.peers[k].pack_subs
    if which == 2:
        return plan.peers[k].unpack_subs
    raise ValueError(f"bad which {which}")


def _field_desc(plan: TransposePlan, n: int, f: int, which: int, k: int,
                s: int) -> CopyDesc:
    """Sub-block ``s`` of ``(which, k)`` for field ``f`` of ``n``: its
    descriptor with the staging side (dst of a pack, src of an unpack) moved
    by :func:`many_shift`; field ``f`` of a block sits at ``n*o_s + f*c_s``."""
    sb = _subs(plan, which, k)[s]
    if which == 0:
        return sb
    d, sh = sb.desc, many_shift(n, f, sb.offset, sb.nelem)
    if which in (1, 3):
        return CopyDesc(d.dims, d.sstrides, d.soffset, d.dstrides,
                        d.doffset + sh)
    return CopyDesc(d.dims, d.sstrides, d.soffset + sh, d.dstrides, d.doffset)


def copydesc_many(plan: TransposePlan, n: int, f: int, which: int,
                  k: int = 0) -> Optional[CopyDesc]:
    """The descriptor of field ``f`` of ``n`` on an ordinary plan; ``which``
    as in ``pa_plan_copydesc``: 0 local, 1 pack of peer k, 2 unpack of peer k,
    3 staged self pack, 4 staged self unpack.  None where the plan has no
    such descriptor, and on a keep plan (see :func:`copydesc_sub`)."""
    _check_many(n, f)
    if not _subs(plan, which, k) or plan.keep is not None:
        return None
    return _field_desc(plan, n, f, which, k, 0)


def nsub(plan: TransposePlan, which: int, k: int = 0) -> int:
    """Sub-boxes behind ``which`` (as in :func:`copydesc_many`) of a keep
    plan; peer ``k`` for packs and unpacks."""
    if plan.keep is None:
        raise ValueError("not a keep plan")
    subs = _subs(plan, which, k)
    return 0 if subs is None else len(subs)


def copydesc_sub(plan: TransposePlan, n: int, f: int, which: int, k: int,
                 s: int) -> Optional[CopyDesc]:
    """Sub-box ``s`` of field ``f`` of ``n`` on a keep plan, ``which`` as in
    :func:`copydesc_many`; None past the last sub-box."""
    _check_many(n, f)
    if not 0 <= s < nsub(plan, which, k):
        return None
    return _field_desc(plan, n, f, which, k, s)


def stage_descs(plan: TransposePlan, n: int, f: int, stage: int):
    """``(which, desc)`` for every copy that ``stage`` (0 pack, 1 local,
    2 unpack) runs for field ``f`` of ``n``, in launch order, on any plan."""
    if stage == 0:
        blocks = [(1, blk.peer_k) for blk in plan.peers] + [(3, 0)]
    elif stage == 1:
        blocks = [(0, 0), (4, 0)]
    else:
        blocks = [(2, blk.peer_k) for blk in plan.peers]
    return [(which, _field_desc(plan, n, f, which, k, s))
            for which, k in blocks
            for s in range(len(_subs(plan, which, k)))]


def buffer_nelem_many(plan: TransposePlan, n: int) -> Tuple[int, int]:
    """(send, recv) staging sizes in elements for ``n`` fields."""
    _check_many(n)
    return n * plan.send_nelem_total, n * plan.recv_nelem_total


def peer_message(plan: TransposePlan, n: int,
                 k: int) -> Tuple[int, int, int, int]:
    """``(send_off, send_n, recv_off, recv_n)`` in elements of the one message
    exchanged with subgroup peer ``k`` for ``n`` fields; all zero for the
    self block, which is never a message."""
    _check_many(n)
    if plan.r_dim is None or not 0 <= k < len(plan.peers):
        raise ValueError(f"no peer block {k}")
    if k == plan.my_k:
        return (0, 0, 0, 0)
    blk = plan.peers[k]
    return (n * blk.send_offset, n * blk.send_nelem,
            n * blk.recv_offset, n * blk.recv_nelem)
