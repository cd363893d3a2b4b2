"""Helpers of the launch-geometry tests (test_gpu_launch_geometry.py):
descriptors whose workgroup count passes the gridDim.x limit, windows that
sit far into a huge buffer, and the chunked device-side compares that keep a
multi-GiB check from allocating a second buffer of that size.

Host buffers are raw ``uint8`` arrays; an element of ``B`` bytes is viewed as
an unsigned integer, ``complex128`` (16 bytes, moved as bits) or a void type.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from many_util import ceil_div, expected_workgroups
from pencilarrays_amd import native
from wire_gpu_util import ref_conv, side_types, source_values
from wire_util import PAIRS, assert_same

SENT = 0xAB
CH = 1 << 28      # bytes per chunk of a device-side compare
SLACK = 4         # elements behind the last one a descriptor writes
DEV = "cuda:0"


def max_x(threads: int) -> int:
    """Largest gridDim.x of a launch with ``threads`` per workgroup: the
    dispatch limit of 2^32 - 1 work-items per grid dimension."""
    return 0xFFFFFFFF // threads


def elem_dtype(B: int) -> np.dtype:
    """A numpy type of ``B`` bytes that assignment moves as opaque bits."""
    return np.dtype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64,
                     16: np.complex128}.get(B, f"V{B}"))


def host_random(nbytes: int, seed: int) -> np.ndarray:
    """``nbytes`` random bytes (drawn as 64-bit words: a GiB takes well under
    a second)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 64, ceil_div(nbytes, 8), dtype=np.uint64,
                     endpoint=False)
    return w.view(np.uint8)[:nbytes]


def extent(dims, strides, offset: int) -> int:
    """Elements a buffer needs to hold every index the descriptor touches."""
    return offset + 1 + sum((n - 1) * s for n, s in zip(dims, strides))


def host_ref(desc, src: np.ndarray, dst: np.ndarray, B: int) -> None:
    """The descriptor (element units, ``B``-byte elements) on ``uint8`` host
    buffers, as one numpy strided assignment."""
    dims, sstr, soff, dstr, doff = desc
    ast = np.lib.stride_tricks.as_strided
    dt = elem_dtype(B)
    shape = tuple(dims)[::-1]
    sv = ast(src.view(dt)[soff:], shape=shape,
             strides=tuple(s * B for s in sstr)[::-1])
    dv = ast(dst.view(dt)[doff:], shape=shape,
             strides=tuple(s * B for s in dstr)[::-1])
    dv[...] = sv


def first_diff(a, b) -> str:
    """Where two equal-length device byte tensors first differ."""
    for lo in range(0, a.numel(), CH):
        ne = a[lo:lo + CH] != b[lo:lo + CH]
        if bool(ne.any()):
            i = lo + int(ne.nonzero()[0].item())
            return f"first difference at byte {i}: {int(a[i])} != {int(b[i])}"
    return "equal"


def dev_equal(a, b) -> bool:
    """``torch.equal`` of two device tensors of the same shape and type, in
    chunks of their first axis: the compare's temporary stays small."""
    assert a.shape == b.shape and a.dtype == b.dtype
    rows = max(1, CH // max(1, a[0].numel() * a.element_size()))
    return all(torch.equal(a[lo:lo + rows], b[lo:lo + rows])
               for lo in range(0, a.shape[0], rows))


def dev_all(t, value: int) -> bool:
    """Every element of a device tensor equals ``value``, in chunks of its
    first axis."""
    if t.numel() == 0:
        return True
    rows = max(1, CH // max(1, t[0].numel() * t.element_size()))
    return all(bool((t[lo:lo + rows] == value).all())
               for lo in range(0, t.shape[0], rows))


def fill_random(t, seed: int) -> None:
    """Random bytes into a device ``uint8`` tensor, in place and in chunks."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    for lo in range(0, t.numel(), CH):
        t[lo:lo + CH].random_(0, 256, generator=g)


def batch_transpose_desc(n: int, nb: int, soff: int = 0, doff: int = 0):
    """``(n, n, nb)``: ``nb`` dense n x n transposes, one workgroup each."""
    return ((n, n, nb), (1, n, n * n), soff, (n, 1, n * n), doff)


def assert_split(wg: int, threads: int, relation: str = "over") -> None:
    """The launch really is on the side of the gridDim.x limit the case is
    about."""
    mx = max_x(threads)
    if relation == "over":
        assert wg > mx, f"{wg} workgroups do not pass the limit {mx}"
    elif relation == "exact":
        assert wg == mx, f"{wg} workgroups are not exactly the limit {mx}"
    else:
        raise AssertionError(relation)


def run_past_split(desc, ssz: int, ncomp: int, want_kind: int, threads: int,
                   seed: int, want_wg=None, relation: str = "over"):
    """Run ``desc`` (elements of ``ncomp`` scalars of ``ssz`` bytes) through
    pa_device_copy.  Before the copy runs: the selection with the real device
    pointers and the workgroup count against the gridDim.x limit of a
    ``threads``-wide workgroup.  After it: the WHOLE 0xAB-prefilled
    destination (slack included) against a numpy strided assignment of the
    same random source bytes."""
    dims, sstr, soff, dstr, doff = desc
    B = ssz * ncomp
    src = host_random(extent(dims, sstr, soff) * B, seed)
    dst_n = extent(dims, dstr, doff) + SLACK
    exp = np.full(dst_n * B, SENT, dtype=np.uint8)
    host_ref(desc, src, exp, B)
    src_t = torch.from_numpy(src).to(DEV)
    dst_t = torch.full((dst_n * B,), SENT, dtype=torch.uint8, device=DEV)
    try:
        k = native.copy_kernel_kind(desc, ssz, src_t.data_ptr(),
                                    dst_t.data_ptr(), ncomp)
        what = f"ssz={ssz} ncomp={ncomp} {desc} {k}"
        assert (k.kind, k.byteified, k.sweep_depth) == (want_kind, 0, 1), what
        wg = expected_workgroups(desc, k, ssz, ncomp)
        assert_split(wg, threads, relation)
        if want_wg is not None:
            assert wg == want_wg, what
        native.device_copy(desc, ssz, src_t.data_ptr(), dst_t.data_ptr(),
                           ncomp=ncomp)
        torch.cuda.synchronize()
        exp_t = torch.from_numpy(exp).to(DEV)
        ok = torch.equal(dst_t, exp_t)
        assert ok, what + " " + first_diff(dst_t, exp_t)
        return k
    finally:
        src_t = dst_t = exp_t = None
        torch.cuda.empty_cache()


POOL = 1 << 16    # distinct source scalars of a converting case past the split
GUARD = 256


def cvt_host_case(desc, pair: str, op: int, nc: int, seed: int):
    """Source scalars and the expected destination scalars (slack and
    sentinel included) of a converting copy of ``desc`` whose element count
    is too large to convert scalar by scalar on the host in test time.  The
    conversion is elementwise, so it commutes with the copy: the references
    of wire_util convert a pool of ``POOL - 1`` seeded values (the pair's
    special values among them) once, every source scalar is a random draw
    from the pool, the descriptor moves the 16-bit draws with the numpy
    strided assignment, and the destination gathers the converted pool.
    Draw ``POOL - 1`` stands for a destination scalar nobody wrote."""
    dims, sstr, soff, dstr, doff = desc
    st, dt = side_types(pair, op)
    fn, _ = ref_conv(pair, op)
    pool = source_values(POOL - 1, pair, op, seed)
    assert pool.dtype == st
    conv = np.empty(POOL, dtype=dt)
    conv.view(np.uint8)[:] = SENT
    conv[:POOL - 1] = fn(pool, pair)
    src_n = extent(dims, sstr, soff) * nc
    dst_n = (extent(dims, dstr, doff) + SLACK) * nc
    draw = np.minimum(host_random(2 * src_n, seed).view(np.uint16), POOL - 2)
    moved = np.full(dst_n, POOL - 1, dtype=np.uint16)
    host_ref(desc, draw.view(np.uint8), moved.view(np.uint8), 2 * nc)
    return pool[draw], conv[moved]


def run_cvt_past_split(desc, pair: str, op: int, nc: int, want_kind: int,
                       threads: int, want_wg: int, seed: int):
    """Run ``desc`` (elements of ``nc`` scalars) through pa_device_copy_wire.
    Before the copy: the selection with the real pointers and the workgroup
    count (one per tile per batch) against the gridDim.x limit.  After it:
    the whole 0xAB-prefilled destination, guard included, against
    ``cvt_host_case``."""
    code = PAIRS[pair][2]
    dt = side_types(pair, op)[1]
    src, exp = cvt_host_case(desc, pair, op, nc, seed)
    s_t = torch.from_numpy(src.view(np.uint8)).to(DEV)
    d_t = torch.full((exp.nbytes + GUARD,), SENT, dtype=torch.uint8,
                     device=DEV)
    try:
        k = native.copy_kernel_kind_wire(desc, code, op, nc, s_t.data_ptr(),
                                         d_t.data_ptr())
        what = f"{pair} op={op} nc={nc} {desc} {k}"
        assert k.kind == want_kind, what
        dims, _, _, dstr, _ = desc
        ta = dstr.index(1)
        wg = ceil_div(dims[0], k.tile_i) * ceil_div(dims[ta], k.tile_j) * \
            (math.prod(dims) // (dims[0] * dims[ta]))
        assert wg == want_wg, what
        assert_split(wg, threads)
        native.device_copy_wire(desc, code, op, nc, s_t.data_ptr(),
                                d_t.data_ptr())
        torch.cuda.synchronize()
        got = d_t.cpu().numpy()
        assert (got[exp.nbytes:] == SENT).all(), what + " guard"
        assert_same(got[:exp.nbytes].view(dt), exp, what)
    finally:
        s_t = d_t = None
        torch.cuda.empty_cache()


# ---- far offsets ---------------------------------------------------------------

class FarWindow:
    """A three-axis window ``(n0, n1, nb)`` between a small buffer and a huge
    one.  The huge side's offset and batch stride are chosen by the case; the
    near side is dense behind a small offset.  ``spans()`` lists, per batch,
    the element range the window covers on the huge side, so the host
    reference and the device compare only ever touch those ranges."""

    def __init__(self, dims, near_strides, near_off, far_strides, far_off,
                 far_side: str):
        self.dims = tuple(dims)
        self.near = (tuple(near_strides), near_off)
        self.far = (tuple(far_strides), far_off)
        self.far_side = far_side

    def desc(self):
        (ns, no), (fs, fo) = self.near, self.far
        if self.far_side == "src":
            return (self.dims, fs, fo, ns, no)
        return (self.dims, ns, no, fs, fo)

    def spans(self):
        fs, fo = self.far
        inner = extent(self.dims[:2], fs[:2], 0)
        return [(fo + b * fs[2], inner) for b in range(self.dims[2])]

    def batch_desc(self, b: int):
        """The 2-D descriptor of batch ``b`` with the huge side's offset moved
        to the start of that batch's span."""
        (ns, no), (fs, fo) = self.near, self.far
        near = (ns[:2], no + b * ns[2])
        far = (fs[:2], 0)
        s, d = (far, near) if self.far_side == "src" else (near, far)
        return (self.dims[:2], s[0], s[1], d[0], d[1])


def check_far_sentinel(huge, spans_bytes) -> None:
    """Every byte of ``huge`` outside the (sorted, disjoint) byte ranges is
    still the sentinel; chunked."""
    pos = 0
    for lo, n in list(spans_bytes) + [(huge.numel(), 0)]:
        assert lo >= pos
        for c in range(pos, lo, CH):
            seg = huge[c:min(c + CH, lo)]
            assert bool((seg == SENT).all()), \
                f"sentinel overwritten in bytes [{c}, {min(c + CH, lo)})"
        pos = lo + n


def far_bytes_needed(win: FarWindow, B: int) -> int:
    lo, n = win.spans()[-1]
    return (lo + n + SLACK) * B


def roundup(x: int, m: int) -> int:
    return -(-x // m) * m


# Copy families of the far-offset cases.  ``shape``: "t" = transposed (src
# unit-stride along axis 0, dst along axis 1), "l" = linear (both along axis
# 0), "g" = no unit-stride src axis.  ``sp`` / ``dp``: row pitch of the source
# and destination.  ``odd_doff``: the destination offset is odd (keeps 8-byte
# elements off the vector-store tile).  Every other offset and every batch
# stride is a multiple of 8 elements, which the packed and the vector-store
# tile accept.
FAR_DIMS = (70, 66, 3)
FAR_FAMILIES = {
    # name: (ssz, ncomp, kind, shape, sp, dp, odd_doff)
    "linear_1B": (1, 1, "LINEAR", "l", 75, 77, False),
    "generic_4B": (4, 1, "GENERIC", "g", 144, 68, False),
    "tile_1B": (1, 1, "TILE", "t", 72, 67, False),
    "tile_2B": (2, 1, "TILE", "t", 72, 67, False),
    "tile_4B": (4, 1, "TILE", "t", 72, 68, False),
    "tile_8B": (8, 1, "TILE", "t", 72, 68, True),
    "tile_16B": (16, 1, "TILE", "t", 72, 68, False),
    "tile_vs": (8, 1, "TILE_VS", "t", 72, 68, False),
    "tile_pk_1B": (1, 1, "TILE_PK", "t", 72, 72, False),
    "tile_pk_2B": (2, 1, "TILE_PK", "t", 72, 72, False),
    "tile_wide_3x2B": (2, 3, "TILE_WIDE", "t", 72, 68, False),
    "tile_wide_5x4B": (4, 5, "TILE_WIDE", "t", 72, 68, False),
}
# converting families: (ncomp, kind, shape, sp, dp)
FAR_CVT = {
    "cvt_linear": (1, "CVT_LINEAR", "l", 76, 72),
    "cvt_tile": (1, "CVT_TILE", "t", 72, 68),
    "cvt_generic": (5, "CVT_GENERIC", "t", 72, 68),
}


def far_window(shape: str, sp: int, dp: int, odd_doff: bool, far_side: str,
               how: str, thresh_elems: int, dims=FAR_DIMS) -> FarWindow:
    """The window of one far-offset case.  ``how`` = "offset": the huge
    side's offset is the first multiple of 8 past ``thresh_elems``; "batch":
    its offset is small and its batch stride carries the last batch past
    ``thresh_elems``."""
    n0, n1, nb = dims
    lead = 2 if shape == "g" else 1
    assert sp >= lead * n0 and dp >= (n0 if shape == "l" else n1)
    s2 = (lead, sp)
    d2 = (1, dp) if shape == "l" else (dp, 1)
    out = {}
    for side, st2 in (("src", s2), ("dst", d2)):
        inner = roundup(extent(dims[:2], st2, 0), 8) + 8
        odd = 1 if (odd_doff and side == "dst") else 0
        if side != far_side:
            out[side] = (st2 + (inner,), 8 + odd)
        elif how == "offset":
            out[side] = (st2 + (inner,), roundup(thresh_elems + 1, 8) + odd)
        else:
            assert how == "batch"
            bstr = roundup(thresh_elems // (nb - 1) + 8, 8)
            assert bstr > inner
            out[side] = (st2 + (bstr,), 8 + odd)
    near = "dst" if far_side == "src" else "src"
    return FarWindow(dims, out[near][0], out[near][1], out[far_side][0],
                     out[far_side][1], far_side)


def run_far(win: FarWindow, Bs: int, Bd: int, huge, make_src, ref, select,
            launch, same, thresh_bytes: int) -> None:
    """One far-offset case.  ``Bs`` / ``Bd``: bytes per element on the source
    and destination side.  ``make_src(n)``: ``n`` source elements as uint8.
    ``ref(desc2d, src_u8, dst_u8)``: the host reference of one batch.
    ``select(desc, sp, dp)`` asserts the selection, ``launch(desc, sp, dp)``
    runs the copy, ``same(got_u8, exp_u8, what)`` asserts equality.  Only the
    window's spans of the huge side are ever uploaded or downloaded; on a
    huge destination everything else must still be the sentinel."""
    desc = win.desc()
    spans = win.spans()
    nb = win.dims[2]
    ns, no = win.near
    near_n = extent(win.dims, ns, no) + SLACK
    Bfar = Bs if win.far_side == "src" else Bd
    need = far_bytes_needed(win, Bfar)
    assert need <= huge.numel(), (need, huge.numel())
    # the case really is past the threshold, on the last batch at least
    assert spans[-1][0] * Bfar > thresh_bytes, (spans, Bfar, thresh_bytes)
    far = huge[:need]
    try:
        if win.far_side == "src":
            exp = np.full(near_n * Bd, SENT, dtype=np.uint8)
            for b, (lo, n) in enumerate(spans):
                sb = make_src(n)
                assert sb.dtype == np.uint8 and sb.size == n * Bs
                far[lo * Bs:(lo + n) * Bs].copy_(torch.from_numpy(sb))
                ref(win.batch_desc(b), sb, exp)
            dst_t = torch.full((near_n * Bd,), SENT, dtype=torch.uint8,
                               device=DEV)
            select(desc, far.data_ptr(), dst_t.data_ptr())
            launch(desc, far.data_ptr(), dst_t.data_ptr())
            torch.cuda.synchronize()
            same(dst_t.cpu().numpy(), exp, f"{desc} near destination")
        else:
            src = make_src(near_n)
            exps = []
            for b, (lo, n) in enumerate(spans):
                e = np.full(n * Bd, SENT, dtype=np.uint8)
                ref(win.batch_desc(b), src, e)
                exps.append(e)
            src_t = torch.from_numpy(src).to(DEV)
            far.fill_(SENT)
            select(desc, src_t.data_ptr(), far.data_ptr())
            launch(desc, src_t.data_ptr(), far.data_ptr())
            torch.cuda.synchronize()
            for b, (lo, n) in enumerate(spans):
                got = far[lo * Bd:(lo + n) * Bd].cpu().numpy()
                same(got, exps[b], f"{desc} batch {b}")
            check_far_sentinel(far, [(lo * Bd, n * Bd) for lo, n in spans])
    finally:
        torch.cuda.synchronize()
