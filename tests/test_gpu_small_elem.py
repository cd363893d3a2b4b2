"""GPU tests for 1- and 2-byte elements (f16/bf16/int16/int8/uint8/bool):
the packed LDS-tile transpose, its scalar-tile fallback and the generic
kernel, bit-exact against the CPU executor / the oracle on integer
bit-pattern views.

Destinations are prefilled with the 0xAB sentinel and compared WHOLE, so a
wide store that spills past its window is caught.  Every case also asserts,
through pa_copy_kernel_kind with the real device pointers, which kernel ran.

The packed tile is 128 x 128 elements (TI x TJ) with V = 8 / esz elements
per 8-byte access; it has one sweep depth, so there is no large-shape case.
"""

import math

import numpy as np
import pytest

import oracle as orc
from pencilarrays_amd import (
    ManyPencilArray, Pencil, PencilArray, Topology, Transposition, build_plan,
)
from pencilarrays_amd.copyexec import apply_copy
from pencilarrays_amd.plan import CopyDesc
from util import SWEEP

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

import ctypes  # noqa: E402

from pencilarrays_amd import native  # noqa: E402

I64 = ctypes.c_int64
TI = TJ = 128
NP_BITS = {1: np.uint8, 2: np.uint16}
# torch has no full uint16 support: 2-byte bit patterns live in int16 tensors
T_BITS = {1: torch.uint8, 2: torch.int16}


def _to_gpu(a: np.ndarray):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _to_np(t, esz):
    return t.cpu().numpy().view(NP_BITS[esz])


def _sentinel(n, esz):
    t = torch.empty(n, dtype=T_BITS[esz], device="cuda:0")
    t.view(torch.uint8).fill_(0xAB)
    return t


def _rand_bits(rng, n, esz):
    return rng.integers(0, 256 ** esz, n, dtype=NP_BITS[esz])


def _dev_copy(desc, esz, src_t, dst_t):
    lib = native.load()
    nd = len(desc.dims)
    st = lib.pa_device_copy(
        nd, (I64 * nd)(*desc.dims), (I64 * nd)(*desc.sstrides),
        I64(desc.soffset), (I64 * nd)(*desc.dstrides), I64(desc.doffset),
        I64(esz), ctypes.c_void_p(src_t.data_ptr()),
        ctypes.c_void_p(dst_t.data_ptr()), None)
    assert st == 0, lib.pa_last_error().decode()


def _kind(desc, esz, src_t, dst_t):
    return native.copy_kernel_kind(desc, esz, src_t.data_ptr(),
                                   dst_t.data_ptr())


def _run_case(rng, esz, n0, nta, nb, s_pitch, soff, d_pitch, doff,
              src_slice=0, dst_slice=0):
    """Transpose-shaped descriptor: src axis 0 unit-stride with row pitch
    ``s_pitch``; dst unit-stride along axis 1 with row pitch ``d_pitch``.
    ``*_slice`` drops that many leading elements from the device tensor, so
    the base pointer moves.  Returns the selected kernel after checking the
    whole destination bit-exactly."""
    desc = CopyDesc(dims=(n0, nta, nb), sstrides=(1, s_pitch, s_pitch * nta),
                    soffset=soff, dstrides=(d_pitch, 1, d_pitch * n0),
                    doffset=doff)
    v = 8 // esz
    src_n = soff + s_pitch * nta * nb
    dst_n = doff + d_pitch * n0 * nb + 2 * v  # slack: spills land in-buffer
    src = _rand_bits(rng, src_n, esz)
    exp = np.empty(dst_n, dtype=NP_BITS[esz])
    exp.view(np.uint8)[:] = 0xAB
    apply_copy(desc, src, exp)
    pad_s = _rand_bits(rng, src_slice, esz)
    src_t = _to_gpu(np.concatenate([pad_s, src]))[src_slice:]
    dst_t = _sentinel(dst_n + dst_slice, esz)[dst_slice:]
    k = _kind(desc, esz, src_t, dst_t)
    _dev_copy(desc, esz, src_t, dst_t)
    torch.cuda.synchronize()
    got = _to_np(dst_t, esz)
    assert np.array_equal(got, exp), \
        f"esz={esz} dims=({n0},{nta},{nb}) pitch=({s_pitch},{d_pitch}) " \
        f"off=({soff},{doff}) slice=({src_slice},{dst_slice}) kind={k}"
    assert k.byteified == 0
    return k


def _extents(v, t):
    return [1, v - 1, v, v + 1, t - 1, t, t + 1, 2 * t + v + 1]


def _up(n, v):
    return (n + v - 1) // v * v


# ---- 1. descriptor boundary sweep ----------------------------------------

@pytest.mark.parametrize("esz", [1, 2])
def test_boundary_sweep_packed_tile(esz):
    """8 x 8 extents around the vector width and the tile edge, batch 3.
    The buffers are dense up to the alignment the packed tile needs: each
    row pitch is the extent rounded up to V (a dense row of V+1 elements
    cannot keep every row 8-byte aligned).  Every descriptor with both
    extents > 1 must run the packed tile; a unit extent drops out of the
    normalized descriptor, which then has no contiguous axis on one side
    (generic kernel)."""
    v = 8 // esz
    rng = np.random.default_rng(100 + esz)
    for n0 in _extents(v, TI):
        for nta in _extents(v, TJ):
            k = _run_case(rng, esz, n0, nta, 3, _up(n0, v), 0,
                          _up(nta, v), 0)
            want = native.KERNEL_TILE_PK if n0 > 1 and nta > 1 \
                else native.KERNEL_GENERIC
            assert (k.kind, k.word_bytes) == (want, esz), (n0, nta, k)


@pytest.mark.parametrize("esz", [1, 2])
def test_boundary_sweep_fully_dense(esz):
    """The same 64 extents with fully dense buffers (pitch == extent): the
    packed tile exactly when both extents are multiples of V, else the
    scalar tile; unit extents collapse to a linear copy."""
    v = 8 // esz
    rng = np.random.default_rng(200 + esz)
    for n0 in _extents(v, TI):
        for nta in _extents(v, TJ):
            k = _run_case(rng, esz, n0, nta, 3, n0, 0, nta, 0)
            if n0 == 1 or nta == 1:
                assert k.kind in (native.KERNEL_COPY_1D,
                                  native.KERNEL_LINEAR), (n0, nta, k)
                continue
            want = native.KERNEL_TILE_PK if n0 % v == 0 and nta % v == 0 \
                else native.KERNEL_TILE
            assert (k.kind, k.word_bytes) == (want, esz), (n0, nta, k)


# ---- 2. misalignment sweep ------------------------------------------------

MISALIGN = ["odd_soff", "odd_sstr", "odd_doff", "odd_dstr", "src_ptr",
            "dst_ptr", "all"]


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("what", MISALIGN)
def test_misaligned_windows_take_scalar_tile(esz, what):
    """Windows of larger parents with odd strides / odd offsets / base
    pointers sliced by one element: each misalignment alone (and all at
    once) must select the scalar tile and stay bit-exact, sentinel intact
    around the window."""
    v = 8 // esz
    rng = np.random.default_rng(300 + esz)
    every = what == "all"
    for n0 in (v + 1, TI + 1):
        for nta in (v + 1, TJ + 1):
            s_pitch = _up(n0, v) + 2 * v
            d_pitch = _up(nta, v) + v
            soff = 3 * v
            doff = 2 * v
            if every or what == "odd_sstr":
                s_pitch += 1
            if every or what == "odd_dstr":
                d_pitch += 1
            if every or what == "odd_soff":
                soff += 1
            if every or what == "odd_doff":
                doff += 1
            ss = 1 if every or what == "src_ptr" else 0
            ds = 1 if every or what == "dst_ptr" else 0
            k = _run_case(rng, esz, n0, nta, 3, s_pitch, soff, d_pitch, doff,
                          ss, ds)
            assert (k.kind, k.word_bytes) == (native.KERNEL_TILE, esz), \
                (what, n0, nta, k)


@pytest.mark.parametrize("esz", [1, 2])
def test_aligned_windows_take_packed_tile(esz):
    """The aligned twin of the misalignment sweep: windows of larger parents
    whose pitches and offsets are multiples of V run the packed tile and
    leave the parent outside the window untouched."""
    v = 8 // esz
    rng = np.random.default_rng(400 + esz)
    for n0 in (v + 1, TI + 1):
        for nta in (v + 1, TJ + 1):
            k = _run_case(rng, esz, n0, nta, 3, _up(n0, v) + 2 * v, 3 * v,
                          _up(nta, v) + v, 2 * v)
            assert (k.kind, k.word_bytes) == (native.KERNEL_TILE_PK, esz)


# ---- 3. end-to-end world-1 Transposition.execute --------------------------

DTYPES = ["float16", "bfloat16", "int16", "int8", "uint8", "bool"]
E2E = [(dims, perm, ()) for dims in [(42, 31, 29), (64, 64, 64),
                                     (130, 66, 34)]
       for perm in [(1, 2, 0), (2, 0, 1)]] + [((24, 18, 12), (1, 2, 0), (3,))]

_ORACLE_CACHE = {}


def _e2e_reference(dims, perm, extra, esz):
    """(src bits, expected dst bits), computed once per shape and width and
    shared by every dtype of that width; never modified."""
    key = (dims, perm, extra, esz)
    if key not in _ORACLE_CACHE:
        topo = Topology((1, 1))
        n = Pencil(topo, dims, (1, 2)).length_local(0) * \
            math.prod(extra or (1,))
        rng = np.random.default_rng(hash(key) & 0xFFFF)
        src = _rand_bits(rng, n, esz)
        exp = orc.transpose_oracle([src], dims, (1, 1), (1, 2), (0, 1, 2),
                                   (0, 2), perm, extra)[0]
        src.setflags(write=False)
        exp.setflags(write=False)
        _ORACLE_CACHE[key] = (src, exp)
    return _ORACLE_CACHE[key]


def _packed_ok(desc, esz, sp, dp):
    """The documented fast-path rule, restated: with V = 8/esz, both
    offsets, every src stride but axis 0's, every dst stride but the unit
    one, and both base addresses (in elements) are multiples of V."""
    dims, sstr, soff, dstr, doff = desc
    v = 8 // esz
    assert sstr[0] == 1 and 1 in dstr[1:]
    ta = 1 + dstr[1:].index(1)
    vals = [soff, doff, sp // esz, dp // esz] + list(sstr[1:]) + \
        [d for a, d in enumerate(dstr) if a != ta]
    return all(x % v == 0 for x in vals) and sp % esz == 0 and dp % esz == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", E2E, ids=lambda c: f"{c[0]}p{c[1]}e{c[2]}")
def test_world1_execute_small_dtypes(cfg, dtype):
    dims, perm, extra = cfg
    tdt = getattr(torch, dtype)
    esz = torch.empty(0, dtype=tdt).element_size()
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=perm)
    src_np, exp = _e2e_reference(dims, perm, extra, esz)
    src = PencilArray.empty(Pi, 0, dtype=dtype, extra_dims=extra,
                            device="cuda")
    dst = PencilArray.empty(Po, 0, dtype=dtype, extra_dims=extra,
                            device="cuda")
    assert src.data.is_cuda and src.data.dtype == tdt
    src.data.view(T_BITS[esz]).copy_(_to_gpu(src_np))
    dst.data.view(torch.uint8).fill_(0xAB)

    t = Transposition(dst, src)
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None  # ran through the native engine
    got = _to_np(dst.data.view(T_BITS[esz]), esz)
    assert np.array_equal(got, exp)

    k = native.copy_kernel_kind(t._native.native.copydesc(0), esz,
                                src.data.data_ptr(), dst.data.data_ptr())
    desc = t._native.native.copydesc(0)
    packed = _packed_ok(desc, esz, src.data.data_ptr(), dst.data.data_ptr())
    assert packed == (dims == (64, 64, 64) or bool(extra))
    assert k.kind == (native.KERNEL_TILE_PK if packed
                      else native.KERNEL_TILE), k
    assert (k.word_bytes, k.byteified) == (esz, 0)


# ---- 4. in-place round trip -----------------------------------------------

@pytest.mark.parametrize("dtype", ["float16", "int8"])
def test_inplace_roundtrip_small_dtypes(dtype):
    dims = (64, 48, 40)
    tdt = getattr(torch, dtype)
    esz = torch.empty(0, dtype=tdt).element_size()
    topo = Topology((1, 1))
    p1 = Pencil(topo, dims, (1, 2))
    p2 = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    m = ManyPencilArray([p1, p2], 0, dtype=dtype, device="cuda")
    x, y = m[0], m[1]
    assert x.data.is_cuda and x.data.dtype == tdt
    rng = np.random.default_rng(11)
    src_np = _rand_bits(rng, p1.length_local(0), esz)
    x.data.view(T_BITS[esz]).copy_(_to_gpu(src_np))
    t = Transposition(y, x)
    assert t.aliased
    t.execute()
    torch.cuda.synchronize()
    assert t._native is not None
    exp = orc.transpose_oracle([src_np], dims, (1, 1), (1, 2), (0, 1, 2),
                               (0, 2), (1, 2, 0), ())[0]
    assert np.array_equal(_to_np(y.data.view(T_BITS[esz]), esz), exp)
    t2 = Transposition(x, y)
    assert t2.aliased
    t2.execute()
    torch.cuda.synchronize()
    assert np.array_equal(_to_np(x.data.view(T_BITS[esz]), esz), src_np)


# ---- 5. multi-rank simulation on one GPU ----------------------------------

MULTI_PERMUTED = [SWEEP[0], SWEEP[4]]


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("cfg", MULTI_PERMUTED,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_multirank_sim_small_elements(cfg, esz):
    """Full multi-rank permuted transpose on one GPU with int16 / uint8
    data: real pack and unpack windows through the native kernels,
    device-to-device copies standing in for the exchange."""
    dims, pdims, di, pi, do, po, extra, _ = cfg
    assert math.prod(pdims) > 1 and tuple(po) != tuple(range(len(dims)))
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    rng = np.random.default_rng(500 + esz)
    g = _rand_bits(rng, math.prod(dims), esz).reshape(dims)
    nr = topo.nranks
    parents = [orc.parent_from_global(g, dims, pdims, di, pi, r, extra)
               for r in range(nr)]

    plans = [build_plan(Pi, Po, r, extra) for r in range(nr)]
    srcs = [_to_gpu(parents[r]) for r in range(nr)]
    dsts = [_sentinel(Po.length_local(r), esz) for r in range(nr)]
    sends = [_sentinel(max(p.send_nelem_total, 1), esz) for p in plans]
    recvs = [_sentinel(max(p.recv_nelem_total, 1), esz) for p in plans]
    kinds = set()

    def run(desc, s, d):
        kinds.add(_kind(desc, esz, s, d).kind)
        assert _kind(desc, esz, s, d).byteified == 0
        _dev_copy(desc, esz, s, d)

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
            q = plans[blk.global_rank]
            rblk = q.peers[p.my_k]
            recvs[blk.global_rank][rblk.recv_offset:
                                   rblk.recv_offset + rblk.recv_nelem] = \
                sends[r][blk.send_offset:blk.send_offset + blk.send_nelem]
    for r, p in enumerate(plans):
        for blk in p.peers:
            if blk.unpack is not None:
                run(blk.unpack, recvs[r], dsts[r])
    torch.cuda.synchronize()

    exp = orc.transpose_oracle(parents, dims, pdims, di, pi, do, po, extra)
    for r in range(nr):
        assert np.array_equal(_to_np(dsts[r], esz), exp[r]), f"rank {r}"
    # the permuted unpack is a transpose: a tile kernel must have run
    assert kinds & {native.KERNEL_TILE, native.KERNEL_TILE_PK}, kinds


# ---- 6. generic path -------------------------------------------------------

@pytest.mark.parametrize("esz", [1, 2])
def test_generic_kernel_small_elements(esz):
    """No contiguous axis on the src side: the generic gather/scatter kernel
    in esz-byte words (not the byte-ify fallback)."""
    n0, n1, n2 = 37, 21, 5
    desc = CopyDesc(dims=(n0, n1, n2), sstrides=(2, 2 * n0 + 3,
                                                 (2 * n0 + 3) * n1),
                    soffset=1, dstrides=(n1, 1, n0 * n1 + 7), doffset=3)
    rng = np.random.default_rng(600 + esz)
    src = _rand_bits(rng, 1 + (2 * n0 + 3) * n1 * n2, esz)
    exp = np.empty(3 + (n0 * n1 + 7) * n2, dtype=NP_BITS[esz])
    exp.view(np.uint8)[:] = 0xAB
    apply_copy(desc, src, exp)
    src_t = _to_gpu(src)
    dst_t = _sentinel(exp.size, esz)
    k = _kind(desc, esz, src_t, dst_t)
    assert (k.kind, k.word_bytes, k.byteified) == \
        (native.KERNEL_GENERIC, esz, 0)
    _dev_copy(desc, esz, src_t, dst_t)
    torch.cuda.synchronize()
    assert np.array_equal(_to_np(dst_t, esz), exp)
