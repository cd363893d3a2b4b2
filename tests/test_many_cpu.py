"""Multi-field transposes, host side (no GPU): the n-field staging layout,
native vs Python plan parity, the launch plan of the grouped stages, and
MultiTransposition on numpy arrays."""

from __future__ import annotations

import math

import numpy as np
import pytest

from many_util import expected_dests, expected_workgroups, random_parents
from util import SWEEP

from pencilarrays_amd import (
    MultiTransposition,
    Pencil,
    PencilArray,
    Topology,
    Transposition,
    build_plan,
    native,
    run_transpose_sim,
    run_transpose_sim_many,
    transpose_many_into,
)
from pencilarrays_amd.plan import (
    buffer_nelem_many,
    copydesc_many,
    peer_message,
)

# chain, unsorted decomp (#57), uneven grid, local permutation, extra dims
# (one and two), slab, empty ranks, decomposition incl. dim 0, 4-D
SUBSET = [SWEEP[i] for i in (0, 3, 4, 6, 8, 9, 11, 13, 14, 18, 19)]


def _ids(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}_e{c[6]}"


def _arrays(P, parents_f, dtype, extra, elem_dims=()):
    return [PencilArray(P, r, parents_f[r].view(dtype).copy(), extra,
                        elem_dims) for r in range(len(parents_f))]


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("cfg", SUBSET, ids=_ids)
def test_offset_rule_vs_oracle(cfg, n, oracle_lib_path):
    dims, pdims, di, pi, do, po, extra, dtype = cfg
    esz = np.dtype(dtype).itemsize
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    parents = random_parents(dims, pdims, di, extra, esz, n, oracle_lib_path)
    exp = expected_dests(parents, (dims, pdims, di, pi, do, po, extra), esz,
                         oracle_lib_path)
    srcs = [_arrays(Pi, parents[f], dtype, extra) for f in range(n)]
    dsts = [[PencilArray(Po, r, np.zeros(len(exp[f][r]) // esz, dtype=dtype),
                         extra) for r in range(nr)] for f in range(n)]
    staging = {}
    run_transpose_sim_many([[dsts[f][r] for f in range(n)] for r in range(nr)],
                           [[srcs[f][r] for f in range(n)] for r in range(nr)],
                           staging_out=staging)
    for f in range(n):
        for r in range(nr):
            assert dsts[f][r].data.view(np.uint8).tobytes() == \
                exp[f][r].tobytes(), (f, r)
    if n == 1:
        one = {}
        d1 = [PencilArray(Po, r, np.zeros(len(exp[0][r]) // esz, dtype=dtype),
                          extra) for r in range(nr)]
        run_transpose_sim(d1, srcs[0], staging_out=one)
        for r in range(nr):
            for side in ("send", "recv"):
                assert staging[side][r].tobytes() == one[side][r].tobytes()


def _native_cases():
    out = []
    for cfg in SUBSET:
        out.append((cfg, False, 1))
    out.append((SWEEP[0], True, 1))   # aliased, distributed
    out.append((SWEEP[6], True, 1))   # aliased, same decomposition
    out.append((SWEEP[0], False, 3))  # elem_dims = (3,)
    out.append((SWEEP[0], True, 3))
    return out


@pytest.mark.parametrize("cfg,aliased,ncomp", _native_cases(),
                         ids=lambda v: _ids(v) if isinstance(v, tuple)
                         else str(v))
def test_native_matches_python(cfg, aliased, ncomp):
    dims, pdims, di, pi, do, po, extra, dtype = cfg
    ssz = np.dtype(dtype).itemsize
    esz = ssz * ncomp
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    for r in range(topo.nranks):
        pl = build_plan(Pi, Po, r, extra, aliased=aliased)
        npl = native.NativePlan(Pi, Po, r, ssz, extra, aliased=aliased,
                                ncomp=ncomp)
        for n in (1, 2, 3):
            s, rcv = buffer_nelem_many(pl, n)
            assert npl.buffer_sizes_many(n) == (s * esz, rcv * esz)
            if n == 1:
                assert npl.buffer_sizes_many(1) == npl.buffer_sizes()
            for k in range(len(pl.peers)):
                assert npl.peer_message(n, k) == tuple(
                    v * esz for v in peer_message(pl, n, k))
            for f in range(n):
                for which in range(5):
                    for k in range(max(1, len(pl.peers))):
                        a = copydesc_many(pl, n, f, which, k)
                        b = npl.copydesc_many(n, f, which, k)
                        if a is None:
                            assert b is None, (r, n, f, which, k)
                        else:
                            assert b == (a.dims, a.sstrides, a.soffset,
                                         a.dstrides, a.doffset), \
                                (r, n, f, which, k)
                        if n == 1 and which != 0:
                            assert b == npl.copydesc(which, k)
    # blocks tile the n-fold buffers: field slots are disjoint and cover
    n = 3
    pl = build_plan(Pi, Po, 0, extra, aliased=aliased)
    if pl.r_dim is not None:
        seen = np.zeros(buffer_nelem_many(pl, n)[0], dtype=np.int32)
        for blk in pl.peers:
            for f in range(n):
                d = copydesc_many(pl, n, f, 1, blk.peer_k)
                if d is not None:
                    seen[d.doffset:d.doffset + d.nelem] += 1
        assert (seen == 1).all()


@pytest.mark.parametrize("cfg", SUBSET, ids=_ids)
def test_sender_receiver_symmetry(cfg):
    dims, pdims, di, pi, do, po, extra, dtype = cfg
    esz = np.dtype(dtype).itemsize
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    plans = [native.NativePlan(Pi, Po, r, esz, extra)
             for r in range(topo.nranks)]
    pyplans = [build_plan(Pi, Po, r, extra) for r in range(topo.nranks)]
    for n in (1, 3):
        for r, pl in enumerate(pyplans):
            for blk in pl.peers:
                if blk.peer_k == pl.my_k:
                    assert plans[r].peer_message(n, blk.peer_k) == (0,) * 4
                    continue
                send = plans[r].peer_message(n, blk.peer_k)
                back = plans[blk.global_rank].peer_message(n, pl.my_k)
                assert send[1] == back[3], (n, r, blk.peer_k)
                assert send[1] == n * blk.send_nelem * esz


# ---- launch plan -------------------------------------------------------

def _slab_plan(dims, esz, P=8, rank=0, ncomp=1, permuted=True):
    topo = Topology((P,))
    Pi = Pencil(topo, dims, (1,))
    Po = Pencil(topo, dims, (0,), permute=(1, 0, 2) if permuted else None)
    return native.NativePlan(Pi, Po, rank, esz, (), ncomp=ncomp)


def _sum_grids(pl, n, which, esz, ncomp=1, dst_ptrs=None, src_ptrs=None):
    """Sum of the single-descriptor grids of every peer descriptor `which`
    of every field."""
    tot = 0
    for f in range(n):
        for k in range(pl.nproc_sub):
            d = pl.copydesc_many(n, f, which, k)
            if d is None:
                continue
            kk = native.copy_kernel_kind(
                d, esz, src_ptrs[f] if src_ptrs else 256,
                dst_ptrs[f] if dst_ptrs else 256, ncomp=ncomp)
            tot += expected_workgroups(d, kk, esz, ncomp)
    return tot


def test_launch_plan_even_slab():
    n, esz = 3, 8
    pl = _slab_plan((64, 64, 64), esz)
    pack = pl.stage_launches(n, native.STAGE_PACK)
    assert len(pack) == 1
    assert (pack[0].kind, pack[0].grouped, pack[0].entries) == \
        (native.KERNEL_LINEAR, True, 21)
    assert pack[0].workgroups == _sum_grids(pl, n, 1, esz)
    unpack = pl.stage_launches(n, native.STAGE_UNPACK)
    assert len(unpack) == 1
    assert (unpack[0].kind, unpack[0].grouped, unpack[0].entries) == \
        (native.KERNEL_TILE_VS, True, 21)
    assert unpack[0].workgroups == _sum_grids(pl, n, 2, esz)
    local = pl.stage_launches(n, native.STAGE_LOCAL)
    assert [(l.kind, l.grouped, l.entries) for l in local] == \
        [(native.KERNEL_TILE_VS, True, 3)]


def test_launch_plan_odd_extents_take_scalar_tile():
    n, esz = 3, 8
    pl = _slab_plan((65, 63, 5), esz)
    unpack = pl.stage_launches(n, native.STAGE_UNPACK)
    assert [(l.kind, l.grouped, l.entries) for l in unpack] == \
        [(native.KERNEL_TILE, True, 21)]
    assert unpack[0].workgroups == _sum_grids(pl, n, 2, esz)
    pack = pl.stage_launches(n, native.STAGE_PACK)
    assert len(pack) == 1 and pack[0].grouped and pack[0].entries == 21
    assert pack[0].workgroups == _sum_grids(pl, n, 1, esz)


def test_launch_plan_misaligned_field_moves_alone():
    n, esz = 3, 8
    pl = _slab_plan((64, 64, 64), esz)
    dsts = [0x10000, 0x20008, 0x30000]  # field 1: 8 mod 16, no 16-B stores
    unpack = pl.stage_launches(n, native.STAGE_UNPACK, None, dsts)
    assert [(l.kind, l.grouped, l.entries) for l in unpack] == \
        [(native.KERNEL_TILE_VS, True, 14), (native.KERNEL_TILE, True, 7)]
    assert sum(l.workgroups for l in unpack) == \
        _sum_grids(pl, n, 2, esz, dst_ptrs=dsts)


def test_launch_plan_ungrouped_kinds():
    n = 2
    pl = _slab_plan((64, 64, 64), 2)  # int16 / f16: packed tile
    unpack = pl.stage_launches(n, native.STAGE_UNPACK)
    assert len(unpack) == 14
    assert all((l.kind, l.grouped, l.entries) ==
               (native.KERNEL_TILE_PK, False, 1) for l in unpack)
    assert sum(l.workgroups for l in unpack) == _sum_grids(pl, n, 2, 2)
    pack = pl.stage_launches(n, native.STAGE_PACK)
    assert [(l.kind, l.grouped, l.entries) for l in pack] == \
        [(native.KERNEL_LINEAR, True, 14)]

    pl = _slab_plan((64, 64, 64), 4, ncomp=3)  # 3 x f32: wide tile
    unpack = pl.stage_launches(n, native.STAGE_UNPACK)
    assert len(unpack) == 14
    assert all((l.kind, l.grouped, l.entries) ==
               (native.KERNEL_TILE_WIDE, False, 1) for l in unpack)
    assert sum(l.workgroups for l in unpack) == \
        _sum_grids(pl, n, 2, 4, ncomp=3)


def test_launch_plan_empty_rank_has_no_blocks():
    dims, pdims, di, pi, do, po, extra, dtype = SWEEP[13]
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    # rank 6 owns nothing of dim 0 (3 over 4 ranks) in the input pencil
    r = next(r for r in range(topo.nranks) if Pi.length_local(r) == 0)
    pl = native.NativePlan(Pi, Po, r, 8, extra)
    assert pl.stage_launches(3, native.STAGE_PACK) == []
    assert pl.stage_launches(3, native.STAGE_LOCAL) == []


def test_many_errors():
    pl = _slab_plan((64, 64, 64), 8)
    with pytest.raises(RuntimeError, match="n must be >= 1"):
        pl.buffer_sizes_many(0)
    with pytest.raises(RuntimeError, match="n must be >= 1"):
        pl.peer_message(0, 1)
    with pytest.raises(RuntimeError, match="no peer block"):
        pl.peer_message(2, 8)
    with pytest.raises(RuntimeError, match="n must be >= 1"):
        pl.stage_launches(0, native.STAGE_PACK)
    assert pl.copydesc_many(2, 2, 1, 1) is None  # field out of range
    # stages refuse to run without staging buffers / with null pointers;
    # both are rejected before anything touches a device
    with pytest.raises(RuntimeError, match="missing staging buffers"):
        pl.pack_many([0x1000, 0x2000])
    pl.set_buffers(0x100000, 0x200000)
    with pytest.raises(RuntimeError, match="null src pointer for field 1"):
        pl.pack_many([0x1000, 0])
    with pytest.raises(RuntimeError, match="null dst pointer for field 0"):
        pl.unpack_many([0, 0x1000])
    with pytest.raises(RuntimeError, match="requires pa_plan_set_comm"):
        pl.execute_many([0x1000], [0x2000])
    pl.set_buffers(0, 0)


# ---- MultiTransposition on numpy ----------------------------------------

def _world1(dims=(12, 10, 9), po=(1, 2, 0)):
    topo = Topology((1, 1))
    return (Pencil(topo, dims, (1, 2)),
            Pencil(topo, dims, (0, 2), permute=po))


def test_multi_numpy_matches_singles():
    Pi, Po = _world1()
    rng = np.random.default_rng(3)
    n = 3
    srcs = [PencilArray(Pi, 0, rng.standard_normal(Pi.length_local(0)))
            for _ in range(n)]
    dsts = [PencilArray(Po, 0, np.zeros(Po.length_local(0)))
            for _ in range(n)]
    ref = [PencilArray(Po, 0, np.zeros(Po.length_local(0)))
           for _ in range(n)]
    out = MultiTransposition(dsts, srcs).execute()
    assert out is not None and len(out) == n
    for f in range(n):
        Transposition(ref[f], srcs[f]).execute()
        assert np.array_equal(dsts[f].data, ref[f].data)
    again = [PencilArray(Po, 0, np.zeros(Po.length_local(0)))
             for _ in range(n)]
    transpose_many_into(again, srcs)
    for f in range(n):
        assert np.array_equal(again[f].data, ref[f].data)


def test_multi_numpy_inplace_pairs():
    Pi, Po = _world1()
    rng = np.random.default_rng(4)
    n = 2
    L = max(Pi.length_local(0), Po.length_local(0))
    bufs = [rng.standard_normal(L) for _ in range(n)]
    srcs_np = [b[:Pi.length_local(0)].copy() for b in bufs]
    srcs = [PencilArray(Pi, 0, b[:Pi.length_local(0)]) for b in bufs]
    dsts = [PencilArray(Po, 0, b[:Po.length_local(0)]) for b in bufs]
    mt = MultiTransposition(dsts, srcs)
    assert mt.aliased and mt.plan.aliased
    mt.execute()
    for f in range(n):
        ref = PencilArray(Po, 0, np.zeros(Po.length_local(0)))
        Transposition(ref, PencilArray(Pi, 0, srcs_np[f])).execute()
        assert np.array_equal(dsts[f].data, ref.data)


def test_multi_numpy_cross_alias():
    """Pair 0's destination is pair 1's source: aliasing is detected over
    all pairs, and every source is read before any destination is written."""
    Pi, Po = _world1(dims=(6, 6, 6), po=(0, 1, 2))
    rng = np.random.default_rng(5)
    a = rng.standard_normal(Pi.length_local(0))
    b = rng.standard_normal(Pi.length_local(0))
    a0, b0 = a.copy(), b.copy()
    c = np.zeros(Po.length_local(0))
    mt = MultiTransposition(
        [PencilArray(Po, 0, b), PencilArray(Po, 0, c)],
        [PencilArray(Pi, 0, a), PencilArray(Pi, 0, b)])
    assert mt.aliased
    mt.execute()
    assert np.array_equal(b, a0) and np.array_equal(c, b0)


def test_multi_validation():
    Pi, Po = _world1()
    Pi2, Po2 = _world1(dims=(12, 10, 8))
    z = np.zeros

    def arr(P, dtype=np.float64, extra=(), elem=()):
        return PencilArray(P, 0, z(P.length_local(0) * math.prod(extra or (1,))
                                   * math.prod(elem or (1,)), dtype=dtype),
                           extra, elem)

    with pytest.raises(ValueError, match="same length"):
        MultiTransposition([arr(Po)], [arr(Pi), arr(Pi)])
    with pytest.raises(ValueError, match="at least one field"):
        MultiTransposition([], [])
    with pytest.raises(ValueError, match="source pencil differs"):
        MultiTransposition([arr(Po), arr(Po)], [arr(Pi), arr(Pi2)])
    with pytest.raises(ValueError, match="destination pencil differs"):
        MultiTransposition([arr(Po), arr(Po2)], [arr(Pi), arr(Pi)])
    with pytest.raises(ValueError, match="same backend, dtype and device"):
        MultiTransposition([arr(Po), arr(Po, np.float32)],
                           [arr(Pi), arr(Pi, np.float32)])
    with pytest.raises(ValueError, match="extra dimensions"):
        MultiTransposition([arr(Po), arr(Po, extra=(2,))],
                           [arr(Pi), arr(Pi, extra=(2,))])
    with pytest.raises(ValueError, match="element dimensions"):
        MultiTransposition([arr(Po), arr(Po, elem=(3,))],
                           [arr(Pi), arr(Pi, elem=(3,))])
    with pytest.raises(ValueError, match="same rank"):
        topo = Topology((2, 1))
        A = Pencil(topo, (12, 10, 9), (1, 2))
        B = Pencil(topo, (12, 10, 9), (0, 2))
        MultiTransposition(
            [PencilArray(B, 0, z(B.length_local(0))),
             PencilArray(B, 1, z(B.length_local(1)))],
            [PencilArray(A, 0, z(A.length_local(0))),
             PencilArray(A, 1, z(A.length_local(1)))])
