"""GPU tests for vector-valued elements (``elem_dims`` / the ``*_comp`` C
ABI): the wide-element LDS tile, the reuse of the tuned tiles for
power-of-two totals, and the word-expanded linear fallback — bit-exact
against the numpy executor on opaque B-byte items and the C oracle at
``esz = B``.

Destinations are prefilled with the 0xAB sentinel and compared WHOLE, so a
store past its window is caught.  Every case asserts, through
pa_copy_kernel_kind_comp with the real device pointers, which kernel ran.

The wide tile is 16 elements along ta and, along axis 0, the largest power
of two in 16..256 whose row is at most 1536 bytes (256 for B <= 6, 128 for
12, 64 for 20 and 24, 32 for 32 and 48, 16 for 64); the extents of the
boundary sweep hold t-1, t, t+1 of each of these.
"""

import math

import numpy as np
import pytest

from elem_util import seeded_elem_parents
from pencilarrays_amd import (
    ManyPencilArray, Pencil, PencilArray, Topology, Transposition, build_plan,
)
from pencilarrays_amd.copyexec import apply_copy
from pencilarrays_amd.plan import CopyDesc
from util import SWEEP, COracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402

EXTENTS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256,
           257]
POW2 = (1, 2, 4, 8, 16)


def _word(B, *ptrs):
    """Largest power of two <= 16 dividing B and every address."""
    w = 16
    while w > 1 and (B % w or any(p % w for p in ptrs)):
        w //= 2
    return w


def _void(a_u8, B):
    return a_u8.view(np.dtype((np.void, B)))


def _gpu_bytes(a_u8, lead=0):
    """Device copy of a byte array, ``lead`` bytes into its allocation."""
    t = torch.empty(a_u8.size + lead, dtype=torch.uint8, device="cuda:0")
    t[lead:].copy_(torch.from_numpy(a_u8))
    return t[lead:]


def _sentinel(nbytes, lead=0):
    t = torch.empty(nbytes + lead, dtype=torch.uint8, device="cuda:0")
    t.fill_(0xAB)
    return t[lead:]


def _run_desc(rng, desc, ssz, ncomp, src_n, dst_n, src_lead=0, dst_lead=0):
    """Run ``desc`` (element units) over a random source of ``src_n``
    elements into a sentinel destination of ``dst_n`` elements; check the
    whole destination against the numpy executor.  Returns the kernel."""
    B = ssz * ncomp
    src = rng.integers(0, 256, src_n * B, dtype=np.uint8)
    exp = np.full(dst_n * B, 0xAB, dtype=np.uint8)
    apply_copy(desc, _void(src, B), _void(exp, B))
    src_t = _gpu_bytes(src, src_lead)
    dst_t = _sentinel(dst_n * B, dst_lead)
    k = native.copy_kernel_kind(desc, ssz, src_t.data_ptr(),
                                dst_t.data_ptr(), ncomp=ncomp)
    native.device_copy(desc, ssz, src_t.data_ptr(), dst_t.data_ptr(),
                       ncomp=ncomp)
    torch.cuda.synchronize()
    got = dst_t.cpu().numpy()
    assert np.array_equal(got, exp), \
        f"pair=({ssz},{ncomp}) desc={desc} lead=({src_lead},{dst_lead}) " \
        f"kind={k}"
    assert k.byteified == 0
    return k


def _transpose_desc(n0, nta, nb, ta_axis, s_pad, d_pad, soff, doff):
    """src unit-stride along axis 0; dst unit-stride along ``ta_axis`` (1 or
    2), the remaining axis is the batch.  Returns (desc, src_n, dst_n)."""
    s_pitch = n0 + s_pad
    d_pitch = nta + d_pad
    if ta_axis == 1:
        dims = (n0, nta, nb)
        sstr = (1, s_pitch, s_pitch * nta)
        dstr = (d_pitch, 1, d_pitch * n0)
    else:
        dims = (n0, nb, nta)
        sstr = (1, s_pitch * nta, s_pitch)
        dstr = (d_pitch, d_pitch * n0, 1)
    desc = CopyDesc(dims=dims, sstrides=sstr, soffset=soff, dstrides=dstr,
                    doffset=doff)
    return desc, soff + s_pitch * nta * nb, doff + d_pitch * n0 * nb + 3


# ---- 1. boundary sweep -------------------------------------------------------

# (batch, ta axis, src pad, dst pad, soff, doff)
VARIANTS = [(3, 1, 5, 3, 7, 11), (1, 1, 0, 0, 0, 0), (3, 2, 2, 1, 3, 5),
            (1, 2, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0)]


@pytest.mark.parametrize("ssz,ncomp", [(8, 3), (4, 3), (2, 3), (1, 3),
                                       (16, 2), (4, 5), (16, 3), (16, 4)])
def test_boundary_sweep_wide_tile(ssz, ncomp):
    """Every pair of extents around the tile edges, batch 1 and 3, ta as
    axis 1 and as axis 2, dense and padded pitches, zero and non-zero
    offsets.  Every descriptor with both extents > 1 must run the wide tile.
    A unit extent drops out of the normalized descriptor, which is then no
    transpose: it runs a linear kernel (dense, or the word-expanded
    descriptor), never the byte-ify fallback."""
    B = ssz * ncomp
    W = _word(B)
    rng = np.random.default_rng(1000 + B)
    for nb, ta_axis, s_pad, d_pad, soff, doff in VARIANTS:
        for n0 in EXTENTS:
            for nta in EXTENTS:
                desc, sn, dn = _transpose_desc(n0, nta, nb, ta_axis, s_pad,
                                               d_pad, soff, doff)
                k = _run_desc(rng, desc, ssz, ncomp, sn, dn)
                what = (ssz, ncomp, n0, nta, nb, ta_axis, s_pad, k)
                if n0 > 1 and nta > 1:
                    assert (k.kind, k.word_bytes, k.words_per_element) == \
                        (native.KERNEL_TILE_WIDE, W, B // W), what
                else:
                    assert k.kind in (native.KERNEL_LINEAR,
                                      native.KERNEL_COPY_1D), what


# ---- 2. misaligned base pointers ---------------------------------------------

@pytest.mark.parametrize("ssz,ncomp,src_lead,dst_lead,W", [
    (4, 6, 4, 0, 4), (8, 6, 0, 8, 8), (8, 3, 4, 0, 4), (16, 3, 0, 8, 8),
    (8, 3, 8, 8, 8), (4, 6, 8, 8, 8), (16, 2, 4, 8, 4),
])
def test_misaligned_pointers_lower_the_word(ssz, ncomp, src_lead, dst_lead, W):
    """Base pointers 4 and 8 bytes into their allocation (a sliced tensor):
    the wide tile runs in the narrower word and stays correct."""
    B = ssz * ncomp
    rng = np.random.default_rng(2000 + B + src_lead + dst_lead)
    for n0, nta in [(33, 17), (64, 65), (129, 31)]:
        desc, sn, dn = _transpose_desc(n0, nta, 3, 1, 2, 1, 5, 3)
        k = _run_desc(rng, desc, ssz, ncomp, sn, dn, src_lead, dst_lead)
        assert (k.kind, k.word_bytes, k.words_per_element) == \
            (native.KERNEL_TILE_WIDE, W, B // W), (n0, nta, k)


# ---- 3. fallbacks and reuse ----------------------------------------------------

def test_element_past_64_bytes_runs_word_expanded_linear():
    rng = np.random.default_rng(3000)
    for n0, nta in [(33, 17), (64, 65)]:
        desc, sn, dn = _transpose_desc(n0, nta, 3, 1, 2, 1, 5, 3)
        k = _run_desc(rng, desc, 8, 9, sn, dn)
        assert (k.kind, k.word_bytes, k.words_per_element) == \
            (native.KERNEL_LINEAR, 8, 9)


def test_no_contiguous_axis_runs_word_expanded_linear():
    n0, n1, n2 = 37, 21, 5
    desc = CopyDesc(dims=(n0, n1, n2),
                    sstrides=(2, 2 * n0 + 3, (2 * n0 + 3) * n1), soffset=1,
                    dstrides=(n1, 1, n0 * n1 + 7), doffset=3)
    rng = np.random.default_rng(3100)
    k = _run_desc(rng, desc, 8, 3, 1 + (2 * n0 + 3) * n1 * n2,
                  3 + (n0 * n1 + 7) * n2)
    assert (k.kind, k.word_bytes, k.words_per_element) == \
        (native.KERNEL_LINEAR, 8, 3)


def test_linear_at_element_level():
    """A strided window with axis 0 contiguous on both sides: the linear
    kernels in the widest word that fits, not the wide tile."""
    rng = np.random.default_rng(3200)
    desc = CopyDesc(dims=(33, 16, 3), sstrides=(1, 41, 41 * 16), soffset=2,
                    dstrides=(1, 33, 33 * 16), doffset=0)
    k = _run_desc(rng, desc, 4, 3, 2 + 41 * 16 * 3, 33 * 16 * 3 + 2)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 4)
    desc = CopyDesc(dims=(4096,), sstrides=(1,), soffset=0, dstrides=(1,),
                    doffset=0)
    k = _run_desc(rng, desc, 8, 3, 4096, 4096 + 2)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 16)


@pytest.mark.parametrize("ssz,ncomp", [(4, 2), (8, 2), (4, 4), (2, 2), (1, 2)])
def test_power_of_two_totals_run_the_tuned_tiles(ssz, ncomp):
    B = ssz * ncomp
    rng = np.random.default_rng(3300 + B)
    desc, sn, dn = _transpose_desc(64, 128, 3, 1, 0, 0, 0, 0)
    k = _run_desc(rng, desc, ssz, ncomp, sn, dn)
    plain = native.copy_kernel_kind(desc, B, 0, 0)
    assert tuple(k)[:4] == tuple(plain)[:4]
    assert k.kind in (native.KERNEL_TILE, native.KERNEL_TILE_VS,
                      native.KERNEL_TILE_PK)


# ---- 4. end to end: Transposition.execute on cuda tensors ----------------------

DTYPES = ["float64", "float32", "float16", "complex64", "int8"]
E2E = [
    ((42, 31, 29), (0, 1, 2), (1, 2, 0), ()),
    ((16, 21, 41), (1, 2, 0), (2, 1, 0), ()),
    ((24, 18, 12), (0, 1, 2), (1, 2, 0), (2,)),
]
_REF = {}


def _e2e_reference(oracle_lib_path, dims, pi, po, extra, B):
    """(src bytes, expected dst bytes) for opaque B-byte elements: computed
    once per shape and element size, shared by every dtype / elem_dims of
    that size, never modified."""
    key = (dims, pi, po, extra, B)
    if key not in _REF:
        _, parents = seeded_elem_parents(dims, (1, 1), (1, 2), pi, extra,
                                         np.uint8, (B,), seed=B)
        exp = COracle(oracle_lib_path).transpose_all(
            parents, dims, (1, 1), (1, 2), pi, (0, 2), po, extra, B)[0]
        parents[0].setflags(write=False)
        exp.setflags(write=False)
        _REF[key] = (parents[0], exp)
    return _REF[key]


def _upload(x, a_u8):
    """Fill a cuda PencilArray's flat with the given bytes (the shared
    reference inputs are read-only, so upload a copy)."""
    x.data.view(torch.uint8).copy_(torch.from_numpy(np.array(a_u8)))


def _check_e2e_kernel(t, src, dst, ssz, ncomp):
    desc = t._native.native.copydesc(0)
    sp, dp = src.data.data_ptr(), dst.data.data_ptr()
    k = native.copy_kernel_kind(desc, ssz, sp, dp, ncomp=ncomp)
    B = ssz * ncomp
    assert k.byteified == 0
    if B in POW2:
        assert tuple(k)[:4] == tuple(
            native.copy_kernel_kind(desc, B, sp, dp))[:4]
        assert k.kind in (native.KERNEL_TILE, native.KERNEL_TILE_VS,
                          native.KERNEL_TILE_PK), k
    else:
        W = _word(B, sp, dp)
        assert (k.kind, k.word_bytes, k.words_per_element) == \
            (native.KERNEL_TILE_WIDE, W, B // W), k


@pytest.mark.parametrize("elem", [(3,), (2, 2)], ids=str)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", E2E, ids=lambda c: f"{c[0]}p{c[1]}to{c[2]}e{c[3]}")
def test_world1_execute_elem_dims(cfg, dtype, elem, oracle_lib_path):
    dims, pi, po, extra = cfg
    tdt = getattr(torch, dtype)
    ssz = torch.empty(0, dtype=tdt).element_size()
    ncomp = math.prod(elem)
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2), permute=pi)
    Po = Pencil(topo, dims, (0, 2), permute=po)
    src_np, exp = _e2e_reference(oracle_lib_path, dims, pi, po, extra,
                                 ssz * ncomp)
    src = PencilArray.empty(Pi, 0, dtype=dtype, extra_dims=extra,
                            device="cuda", elem_dims=elem)
    dst = PencilArray.empty(Po, 0, dtype=dtype, extra_dims=extra,
                            device="cuda", elem_dims=elem)
    assert src.data.dtype == tdt and src.data.numel() == ncomp * len(src)
    _upload(src, src_np)
    dst.data.view(torch.uint8).fill_(0xAB)

    t = Transposition(dst, src)
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None and t._native.native.ncomp == ncomp
    assert np.array_equal(dst.data.view(torch.uint8).cpu().numpy(), exp)
    assert np.array_equal(src.data.view(torch.uint8).cpu().numpy(), src_np)
    _check_e2e_kernel(t, src, dst, ssz, ncomp)
    # the views carry the element axes in front
    assert tuple(dst.logical_view().shape) == elem + dims + extra


def test_deferred_wait(oracle_lib_path):
    dims, pi, po, extra = E2E[0]
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2), permute=pi)
    Po = Pencil(topo, dims, (0, 2), permute=po)
    src_np, exp = _e2e_reference(oracle_lib_path, dims, pi, po, extra, 24)
    src = PencilArray.empty(Pi, 0, dtype="float64", device="cuda",
                            elem_dims=(3,))
    dst = src.similar(Po)
    assert dst.elem_dims == (3,) and dst.data.is_cuda
    _upload(src, src_np)
    dst.data.view(torch.uint8).fill_(0xAB)
    t = Transposition(dst, src)
    t.execute(sync=False)
    t.wait()
    assert np.array_equal(dst.data.view(torch.uint8).cpu().numpy(), exp)


def test_inplace_roundtrip(oracle_lib_path):
    dims = (64, 48, 40)
    topo = Topology((1, 1))
    p1 = Pencil(topo, dims, (1, 2))
    p2 = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    m = ManyPencilArray([p1, p2], 0, dtype="float64", device="cuda",
                        elem_dims=(3,))
    x, y = m[0], m[1]
    assert x.data.is_cuda and x.elem_dims == (3,)
    src_np, exp = _e2e_reference(oracle_lib_path, dims, (0, 1, 2), (1, 2, 0),
                                 (), 24)
    _upload(x, src_np)
    t = Transposition(y, x)
    assert t.aliased
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None
    assert np.array_equal(y.data.view(torch.uint8).cpu().numpy(), exp)
    t2 = Transposition(x, y)
    assert t2.aliased
    t2.execute()
    torch.cuda.synchronize()
    assert np.array_equal(x.data.view(torch.uint8).cpu().numpy(), src_np)


# ---- 5. multi-rank simulation on one GPU ---------------------------------------

def test_multirank_sim_vec3_float32(oracle_lib_path):
    """(16,21,41) on 2 x 2 with a permuted output, three float32 per
    element: every rank's pack, local and unpack descriptor through
    pa_device_copy_comp, device copies standing in for the exchange."""
    dims, pdims, di, pi, do, po, extra, _ = SWEEP[0]
    ssz, ncomp = 4, 3
    B = ssz * ncomp
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    _, parents = seeded_elem_parents(dims, pdims, di, pi, extra, np.uint8,
                                     (B,))
    plans = [build_plan(Pi, Po, r, extra) for r in range(nr)]
    srcs = [_gpu_bytes(parents[r]) for r in range(nr)]
    dsts = [_sentinel(Po.length_local(r) * B) for r in range(nr)]
    sends = [_sentinel(max(p.send_nelem_total, 1) * B) for p in plans]
    recvs = [_sentinel(max(p.recv_nelem_total, 1) * B) for p in plans]
    kinds = set()

    def run(desc, s, d):
        k = native.copy_kernel_kind(desc, ssz, s.data_ptr(), d.data_ptr(),
                                    ncomp=ncomp)
        assert k.byteified == 0
        kinds.add(k.kind)
        native.device_copy(desc, ssz, s.data_ptr(), d.data_ptr(),
                           ncomp=ncomp)

    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.pack is not None:
                run(blk.pack, srcs[r], sends[r])
        if p.local is not None:
            run(p.local, srcs[r], dsts[r])
    torch.cuda.synchronize()
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.peer_k == p.my_k or blk.send_nelem == 0:
                continue
            rblk = plans[blk.global_rank].peers[p.my_k]
            recvs[blk.global_rank][
                rblk.recv_offset * B:
                (rblk.recv_offset + rblk.recv_nelem) * B] = \
                sends[r][blk.send_offset * B:
                         (blk.send_offset + blk.send_nelem) * B]
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.unpack is not None:
                run(blk.unpack, recvs[r], dsts[r])
    torch.cuda.synchronize()

    exp = COracle(oracle_lib_path).transpose_all(
        parents, dims, pdims, di, pi, do, po, extra, B)
    for r in range(nr):
        assert np.array_equal(dsts[r].cpu().numpy(), exp[r]), f"rank {r}"
    # the permuted unpack is a transpose of 12-byte elements
    assert native.KERNEL_TILE_WIDE in kinds, kinds
