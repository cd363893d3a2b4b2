"""GPU tests for the 4-, 8- and 16-byte LDS tiles (k_transpose_tile 128x64,
32x32 for 16-byte words; k_transpose_tile_vs 64x128 with 16-byte vector
stores), their sweep depths 8 and 32, and the copy kernels' never-executed
paths (k_copy_generic past its block cap, k_copy_1d_nt with a tail, linear
copies from base pointers that sit one element into an allocation).

Every descriptor case runs through pa_device_copy, asserts kind, word and
sweep depth through pa_copy_kernel_kind with the real device pointers, and
compares the WHOLE 0xAB-prefilled destination (slack after the last element
and the parent outside the window included) bit for bit with the CPU
executor apply_copy, or with a numpy reshape/transpose of the same data
where apply_copy is too slow.  The reference is never another device run.
"""

import numpy as np
import pytest

import oracle as orc
from pencilarrays_amd import Pencil, PencilArray, Topology, Transposition
from pencilarrays_amd.plan import CopyDesc, normalize_desc
from util import seeded_parents

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402
from tile_util import (  # noqa: E402
    NP_BITS, dev_copy, extent, kernel_of, rand_bits, run_desc, same_bytes,
    sentinel_np, transpose_desc,
)

TILE, TILE_VS = native.KERNEL_TILE, native.KERNEL_TILE_VS
COPY_1D, COPY_1D_NT = native.KERNEL_COPY_1D, native.KERNEL_COPY_1D_NT
LINEAR, GENERIC = native.KERNEL_LINEAR, native.KERNEL_GENERIC
NB = 3
SLACK = 4  # elements after the last one written: a spill lands in-buffer


def _edges(t, more=()):
    return sorted({1, 2, t - 1, t, t + 1, 2 * t + 3, *more})


def _run_t(rng, esz, n0, nta, s_pitch, soff, d_pitch, doff, **kw):
    """One transpose-shaped case, batch NB, buffers just large enough plus
    SLACK sentinel elements."""
    want = kw.pop("want", None)
    ss, ds = kw.pop("src_slice", 0), kw.pop("dst_slice", 0)
    desc = transpose_desc(n0, nta, NB, s_pitch, soff, d_pitch, doff, **kw)
    src = rand_bits(rng, extent(desc, desc.sstrides, soff), esz)
    dst_n = extent(desc, desc.dstrides, doff) + SLACK
    return run_desc(desc, esz, src, dst_n, ss, ds, want=want)


# ---- a. boundary sweeps ------------------------------------------------------

def _want_unit(n0, nta, dense, esz, tile_want):
    """A unit extent drops out of the normalized descriptor: dense buffers
    then merge into one contiguous run, a window keeps no axis that is
    unit-stride on both sides (generic kernel)."""
    if n0 > 1 and nta > 1:
        return tile_want
    return None if dense else (GENERIC, esz, 1)


@pytest.mark.parametrize("layout", ["dense", "window"])
def test_boundary_sweep_scalar_tile_esz4(layout):
    """9 x 6 extents around the 128 x 64 tile edges, 4-byte words."""
    rng = np.random.default_rng(1004)
    dense = layout == "dense"
    for n0 in _edges(128, (63, 64, 65)):
        for nta in _edges(64):
            sp, so, dp, do = (n0, 0, nta, 0) if dense else \
                (n0 + 5, 3, nta + 3, 2)
            want = _want_unit(n0, nta, dense, 4, (TILE, 4, 1))
            k = _run_t(rng, 4, n0, nta, sp, so, dp, do, want=want)
            if want is None:
                assert k.kind == COPY_1D, (n0, nta, k)


@pytest.mark.parametrize("layout", ["dense", "window"])
def test_boundary_sweep_scalar_tile_esz8(layout):
    """The same extents in 8-byte words; an odd dst offset keeps every case
    off the vector-store tile."""
    rng = np.random.default_rng(1008)
    dense = layout == "dense"
    for n0 in _edges(128, (63, 64, 65)):
        for nta in _edges(64):
            sp, so, dp, do = (n0, 0, nta, 1) if dense else \
                (n0 + 5, 3, nta + 3, 3)
            want = _want_unit(n0, nta, dense, 8, (TILE, 8, 1))
            k = _run_t(rng, 8, n0, nta, sp, so, dp, do, want=want)
            if want is None:
                assert (k.kind, k.word_bytes) == (COPY_1D, 8), (n0, nta, k)


VS_N0 = [2, 63, 64, 65, 2 * 64 + 3]
VS_NTA = [2, 3, 127, 128, 129, 2 * 128 + 3]


def test_boundary_sweep_vector_store_tile_windows():
    """5 x 6 extents around the 64 x 128 tile edges, windows with even
    pitches and even offsets: all run the vector-store tile.  Odd nta takes
    the scalar tail element, nta = 2, 3 the edge of the even part."""
    rng = np.random.default_rng(1108)
    for n0 in VS_N0:
        for nta in VS_NTA:
            sp = n0 + 4 + (n0 & 1)
            dp = nta + 2 + (nta & 1)
            _run_t(rng, 8, n0, nta, sp, 6, dp, 4, want=(TILE_VS, 8, 1))


def test_boundary_sweep_vector_store_tile_dense():
    """The same extents with dense buffers: a dense row of odd nta has an
    odd pitch, so exactly the even nta run the vector-store tile and the
    odd ones the scalar tile."""
    rng = np.random.default_rng(1208)
    for n0 in VS_N0:
        for nta in VS_NTA:
            kind = TILE if nta & 1 else TILE_VS
            _run_t(rng, 8, n0, nta, n0, 0, nta, 0, want=(kind, 8, 1))


@pytest.mark.parametrize("layout", ["dense", "window"])
def test_boundary_sweep_16_byte_tile(layout):
    """6 x 6 extents around the 32 x 32 tile edges, 16-byte words."""
    rng = np.random.default_rng(1016)
    dense = layout == "dense"
    for n0 in _edges(32):
        for nta in _edges(32):
            sp, so, dp, do = (n0, 0, nta, 0) if dense else \
                (n0 + 5, 3, nta + 3, 1)
            want = _want_unit(n0, nta, dense, 16, (TILE, 16, 1))
            k = _run_t(rng, 16, n0, nta, sp, so, dp, do, want=want)
            if want is None:
                assert (k.kind, k.word_bytes) == (COPY_1D, 16), (n0, nta, k)


# ---- b. each vector-store precondition alone ---------------------------------

# (65, 129, 3) window; every value even unless the case makes it odd
VS_BASE = dict(s_pitch=70, soff=4, d_pitch=132, doff=6,
               s_batch=70 * 129 + 4, d_batch=132 * 65 + 2)
VS_DST = {
    "odd_doff": dict(doff=7),
    "odd_dstr0": dict(d_pitch=133, d_batch=133 * 65 + 1),
    "odd_batch_dstr": dict(d_batch=132 * 65 + 3),
    "dst_ptr": dict(dst_slice=1),
}
VS_SRC = {
    "odd_soff": dict(soff=5),
    "odd_src_pitch": dict(s_pitch=71, s_batch=71 * 129 + 3),
    "src_ptr": dict(src_slice=1),
}


def _vs_case(seed, **over):
    kw = dict(VS_BASE)
    kw.update(over)
    rng = np.random.default_rng(seed)
    return kw, rng


@pytest.mark.parametrize("what", sorted(VS_DST) + ["all_dst"])
def test_vs_each_dst_violation_takes_scalar_tile(what):
    """Odd dst offset, odd dst row pitch, odd dst batch stride, and a dst
    tensor sliced by one element (pointer 8 mod 16): each alone, and all at
    once, must select the scalar tile in 8-byte words and stay bit-exact."""
    over = {}
    for name in (sorted(VS_DST) if what == "all_dst" else [what]):
        over.update(VS_DST[name])
    if what == "all_dst":
        over["d_batch"] = 133 * 65 + 2  # odd pitch and odd batch stride
    kw, rng = _vs_case(1300, **over)
    assert kw["d_batch"] >= kw["d_pitch"] * 65
    _run_t(rng, 8, 65, 129, want=(TILE, 8, 1), **kw)


@pytest.mark.parametrize("what", sorted(VS_SRC) + ["all_src", "all_kept"])
def test_vs_src_misalignment_stays_on_vector_store_tile(what):
    """Only the store side is vectorised: an odd src offset, an odd src
    pitch and a src tensor sliced by one element stay on the vector-store
    tile, as does the window with every condition kept."""
    over = {}
    names = sorted(VS_SRC) if what == "all_src" else \
        [] if what == "all_kept" else [what]
    for name in names:
        over.update(VS_SRC[name])
    kw, rng = _vs_case(1400, **over)
    _run_t(rng, 8, 65, 129, want=(TILE_VS, 8, 1), **kw)


# ---- c. the dst-contiguous axis is not axis 1 --------------------------------

def _four_axis(ta, even):
    """4-axis descriptor, src axis 0 unit-stride, dst unit-stride along axis
    ``ta`` (2 or 3), strided parents on both sides; the other two axes are
    batch axes around ``ta``.  ``even``: every dst stride and offset even
    (vector-store tile); otherwise odd paddings."""
    dims = (65, 5, 129, 3) if ta == 2 else (65, 5, 3, 129)
    p = 2 if even else 3
    sstr, acc = [], 1
    for n in dims:
        sstr.append(acc)
        acc = acc * n + p
    # dst: axis ta fastest, then axis 0, then the batch axes in order
    dstr = [0] * 4
    dstr[ta] = 1
    acc = 129 + (1 if even else 2)
    for a in [0] + [a for a in (1, 2, 3) if a != ta]:
        dstr[a] = acc
        acc = acc * dims[a] + p
    return CopyDesc(dims=dims, sstrides=tuple(sstr), soffset=p + 1,
                    dstrides=tuple(dstr), doffset=2 * p)


@pytest.mark.parametrize("ta", [2, 3])
@pytest.mark.parametrize("esz,kind", [(4, TILE), (8, TILE_VS)])
def test_four_axis_descriptor_ta_not_axis1(esz, kind, ta):
    """Two batch axes go through the a == ta skip of the batch decode, one
    below and one above ta (ta = 2) or both below it (ta = 3), with ragged
    65 x 129 tiles."""
    desc = _four_axis(ta, even=(esz == 8))
    norm = normalize_desc(desc)
    assert len(norm.dims) == 4 and norm.sstrides[0] == 1
    assert norm.dstrides.index(1) == ta
    rng = np.random.default_rng(1500 + 10 * esz + ta)
    src = rand_bits(rng, extent(desc, desc.sstrides, desc.soffset), esz)
    dst_n = extent(desc, desc.dstrides, desc.doffset) + SLACK
    run_desc(desc, esz, src, dst_n, want=(kind, esz, 1))


# ---- d. ragged sweeps at depth 8 and 32 --------------------------------------

# (esz, n0, nta, nb, dst pitch - nta, doff, kind, depth): 67 or 259 tiles
# along ta, so the last chunk is short (takes the break) and the last tile is
# partial.  The thresholds are tile counts: 8 * 4096 and 32 * 4096.
RAGGED = {
    "vs_d8": (8, 2, 66 * 128 + 37, 497, 1, 0, TILE_VS, 8),
    "vs_d32": (8, 2, 258 * 128 + 37, 509, 1, 0, TILE_VS, 32),
    "t8_d8": (8, 3, 66 * 64 + 21, 497, 0, 0, TILE, 8),
    "t8_d32": (8, 2, 258 * 64 + 21, 509, 1, 1, TILE, 32),
    "t4_d8": (4, 3, 66 * 64 + 21, 497, 0, 0, TILE, 8),
    "t4_d32": (4, 3, 258 * 64 + 21, 509, 0, 0, TILE, 32),
    # the shapes above have one tile along axis 0; this one has two (a full
    # 128-row tile next to a 1-row tile), so the block id decodes into tile,
    # chunk and batch with every factor > 1, and full-height tiles reuse the
    # LDS across the sweep (512 MiB each side)
    "t4_d8_tall":(4, 129, 66 * 64 + 21, 245, 0, 0, TILE, 8),
}


@pytest.mark.parametrize("case", sorted(RAGGED))
def test_ragged_sweep(case):
    """The JCHUNK loop with its break, its partial last chunk and the
    barrier between tiles, at depths 8 and 32.  The depth is asserted before
    the copy runs: if a later change moves the thresholds this fails and
    names the shape to re-derive.  Expectation by numpy transpose."""
    esz, n0, nta, nb, pad, doff, kind, depth = RAGGED[case]
    tj = 128 if kind == TILE_VS else 64
    ntj = -(-nta // tj)
    assert ntj % depth and nta % tj, "shape must stay ragged"
    pitch = nta + pad
    desc = transpose_desc(n0, nta, nb, n0, 0, pitch, doff)
    rng = np.random.default_rng(1600)
    src = rng.integers(0, 2 ** (8 * esz), n0 * nta * nb, dtype=NP_BITS[esz],
                       endpoint=False)
    dst_n = doff + pitch * n0 * nb + SLACK
    exp = sentinel_np(dst_n, esz)
    exp[doff:doff + pitch * n0 * nb].reshape(nb, n0, pitch)[:, :, :nta] = \
        src.reshape(nb, nta, n0).transpose(0, 2, 1)
    try:
        run_desc(desc, esz, src, dst_n, exp=exp, want=(kind, esz, depth))
    finally:
        del src, exp
        torch.cuda.empty_cache()


# ---- e. the remaining never-executed paths -----------------------------------

@pytest.mark.parametrize("esz", [4, 8])
def test_generic_kernel_past_block_cap(esz):
    """No unit-stride src axis and 2 * 8192 * 256 + 77 elements: the generic
    kernel's grid is capped at 8192 blocks, so every thread iterates its
    grid-stride loop twice and the first 77 a third time."""
    total = 2 * 8192 * 256 + 77
    n1 = total // 3
    assert 3 * n1 == total
    desc = CopyDesc(dims=(3, n1), sstrides=(2, 6), soffset=1,
                    dstrides=(n1 + 1, 1), doffset=2)
    rng = np.random.default_rng(1700 + esz)
    src = rng.integers(0, 2 ** (8 * esz),
                       extent(desc, desc.sstrides, desc.soffset),
                       dtype=NP_BITS[esz], endpoint=False)
    dst_n = extent(desc, desc.dstrides, desc.doffset) + SLACK
    try:
        run_desc(desc, esz, src, dst_n, want=(GENERIC, esz, 1))
    finally:
        del src
        torch.cuda.empty_cache()


def test_nontemporal_copy_with_tail_and_offsets():
    """512 MiB + 48 bytes of 8-byte elements from element offset 2 to
    element offset 4: the nontemporal copy with a last block that is not
    full.  Compared on the device; sentinel before and after the window."""
    n = (512 << 20) // 8 + 6
    soff, doff, slack = 2, 4, 8
    desc = CopyDesc(dims=(n,), sstrides=(1,), soffset=soff, dstrides=(1,),
                    doffset=doff)
    src = torch.arange(soff + n, dtype=torch.int64, device="cuda:0")
    src.mul_(-7046029254386353131)  # odd multiplier: every element distinct
    dst = torch.empty(doff + n + slack, dtype=torch.int64, device="cuda:0")
    dst.view(torch.uint8).fill_(0xAB)
    try:
        k = kernel_of(desc, 8, src, dst)
        assert (k.kind, k.word_bytes, k.byteified) == (COPY_1D_NT, 16, 0)
        dev_copy(desc, 8, src, dst)
        torch.cuda.synchronize()
        assert torch.equal(dst[doff:doff + n], src[soff:])
        edge = torch.cat([dst[:doff], dst[doff + n:]]).view(torch.uint8)
        assert bool((edge == 0xAB).all())
    finally:
        del src, dst
        torch.cuda.empty_cache()


SHIFTS = {"src": (1, 0), "dst": (0, 1), "both": (1, 1)}
LIN_DESCS = {
    # 4099 elements: 16 * 256 + 3, more than one block at every word
    "run": CopyDesc(dims=(4099,), sstrides=(1,), soffset=0, dstrides=(1,),
                    doffset=0),
    "run16": CopyDesc(dims=(4096,), sstrides=(1,), soffset=16,
                      dstrides=(1,), doffset=32),
    "window": CopyDesc(dims=(64, 37), sstrides=(1, 96), soffset=32,
                       dstrides=(1, 80), doffset=16),
}


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("which", sorted(SHIFTS))
@pytest.mark.parametrize("shape", sorted(LIN_DESCS))
def test_linear_copies_from_sliced_tensors(shape, which, esz):
    """Contiguous runs and a two-axis linear window whose base pointers are
    moved by one element: the word reported (and run) divides both real
    pointers, and the whole buffer is bit-exact."""
    desc = LIN_DESCS[shape]
    ss, ds = SHIFTS[which]
    rng = np.random.default_rng(1800 + esz)
    src = rand_bits(rng, extent(desc, desc.sstrides, desc.soffset), esz)
    dst_n = extent(desc, desc.dstrides, desc.doffset) + 16
    k = run_desc(desc, esz, src, dst_n, ss, ds)
    assert k.kind == (LINEAR if shape == "window" else COPY_1D), k
    w = k.word_bytes
    # torch allocations are at least 256-byte aligned
    assert (ss * esz) % w == 0 and (ds * esz) % w == 0, k
    run_bytes = desc.dims[0] * esz
    widest = next(c for c in (16, 8, 4, 1) if run_bytes % c == 0 and
                  (ss * esz) % c == 0 and (ds * esz) % c == 0)
    assert w == widest, k
    # and the unshifted twin keeps the widest word the run allows
    k0 = run_desc(desc, esz, src, dst_n)
    assert k0.word_bytes == next(c for c in (16, 8, 4, 1)
                                 if run_bytes % c == 0), k0


@pytest.mark.parametrize("dtype", ["float64", "float16"])
def test_world1_identity_transposition_from_offset_source(dtype):
    """World-1 identity-layout Transposition (a straight device copy) whose
    source PencilArray sits one element into its allocation."""
    dims = (42, 31, 29)
    npdt = np.dtype(dtype)
    tdt = getattr(torch, dtype)
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2))
    g, parents = seeded_parents(dims, (1, 1), (1, 2), (0, 1, 2), (), npdt)
    n = parents[0].size
    alloc = torch.empty(n + 1, dtype=tdt, device="cuda:0")
    alloc[1:].copy_(torch.from_numpy(np.ascontiguousarray(parents[0])))
    src = PencilArray(Pi, 0, alloc[1:])
    assert src.data.data_ptr() % 16 == npdt.itemsize
    dst = PencilArray.empty(Po, 0, dtype=dtype, device="cuda")
    dst.data.view(torch.uint8).fill_(0xAB)
    t = Transposition(dst, src)
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None
    exp = orc.transpose_oracle(parents, dims, (1, 1), (1, 2), (0, 1, 2),
                               (0, 2), (0, 1, 2), ())[0]
    assert same_bytes(dst.data.cpu().numpy(), exp)
    k = native.copy_kernel_kind(t._native.native.copydesc(0), npdt.itemsize,
                                src.data.data_ptr(), dst.data.data_ptr())
    assert k.kind == COPY_1D and k.byteified == 0, k
    assert src.data.data_ptr() % k.word_bytes == 0, k
    assert k.word_bytes == (8 if dtype == "float64" else 1), k


# ---- f. end to end with ragged extents and the other word sizes --------------

E2E_DIMS = (130, 67, 35)


def _vs_ok(desc, dp):
    """The documented vector-store rule, restated: 8-byte elements, the dst
    offset and every dst stride but the unit one even, dst pointer 16-byte
    aligned."""
    dims, sstr, soff, dstr, doff = desc
    return doff % 2 == 0 and dp % 16 == 0 and \
        all(d % 2 == 0 for n, d in zip(dims, dstr) if d != 1 and n > 1)


@pytest.mark.parametrize("dtype", ["float32", "complex64", "float64",
                                   "complex128"])
@pytest.mark.parametrize("perm", [(1, 2, 0), (2, 0, 1)], ids=str)
def test_world1_execute_ragged_word_sizes(perm, dtype):
    dims = E2E_DIMS
    npdt = np.dtype(dtype)
    esz = npdt.itemsize
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=perm)
    g, parents = seeded_parents(dims, (1, 1), (1, 2), (0, 1, 2), (), npdt)
    src = PencilArray(
        Pi, 0, torch.from_numpy(np.ascontiguousarray(parents[0])).to("cuda:0"))
    dst = PencilArray.empty(Po, 0, dtype=dtype, device="cuda")
    dst.data.view(torch.uint8).fill_(0xAB)
    t = Transposition(dst, src)
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None  # ran through the native engine
    exp = orc.transpose_oracle(parents, dims, (1, 1), (1, 2), (0, 1, 2),
                               (0, 2), perm, ())[0]
    assert same_bytes(dst.data.cpu().numpy(), exp)

    desc = t._native.native.copydesc(0)
    dp = dst.data.data_ptr()
    k = native.copy_kernel_kind(desc, esz, src.data.data_ptr(), dp)
    want = TILE_VS if esz == 8 and _vs_ok(desc, dp) else TILE
    assert (k.kind, k.word_bytes, k.byteified) == (want, esz, 0), k
