"""Vector-valued elements (``elem_dims``) on the host: PencilArray shapes and
validation, simulated / world-1 / in-place / gloo transposes bit-exact
against the C oracle moving opaque elements of B = ncomp * itemsize bytes,
gather, and the native plan built with ``ncomp``."""

import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from elem_util import c_oracle_elem, same_bits, seeded_elem_parents
from pencilarrays_amd import (
    ManyPencilArray, MPIIOFile, Pencil, PencilArray, Topology, Transposition,
    build_plan, gather_sim, run_transpose_sim,
)
from util import SWEEP

# (elem_dims, scalar dtype)
ELEMS = [((3,), np.float64), ((3,), np.float32), ((2, 2), np.complex64)]
# permuted, unpermuted, uneven 2x3, extra dims, empty ranks, 4-D, world 1
SIM_CFGS = [SWEEP[0], SWEEP[1], SWEEP[2], SWEEP[4], SWEEP[8], SWEEP[9],
            SWEEP[13], SWEEP[18], SWEEP[19], SWEEP[5]]


def _ids(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}e{c[6]}"


# ---- shapes and validation -------------------------------------------------

def test_shapes_views_similar():
    topo = Topology((2, 2))
    dims = (8, 9, 10)
    p = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    rank = 1
    mem = tuple(p.size_local(rank, memory_order=True))
    logical = tuple(p.size_local(rank))
    n = math.prod(mem)
    for elem, extra in [((3,), ()), ((3, 3), ()), ((2,), (4,))]:
        nc = math.prod(elem)
        pex = math.prod(extra)
        flat = np.arange(nc * n * pex, dtype=np.float32)
        x = PencilArray(p, rank, flat, extra_dims=extra, elem_dims=elem)
        assert x.elem_dims == elem and x.ncomp == nc
        assert x.mem_dims == mem + extra
        assert len(x) == n * pex  # elements, not scalars
        mv = x.parent_memview()
        assert mv.shape == elem + mem + extra
        # axis 0 fastest: the components of element 0 are flat[0:nc]
        assert np.array_equal(mv.reshape(-1, order="F"), flat)
        assert mv[(slice(None),) * len(elem) + (0,) * len(mem + extra)] \
            .ravel(order="F").tolist() == list(range(nc))
        lv = x.logical_view()
        assert lv.shape == elem + logical + extra
        assert x.size_local() == logical + extra
        y = x.similar()
        assert y.elem_dims == elem and y.data.shape == flat.shape
        assert y.data.dtype == flat.dtype
        e = PencilArray.empty(p, rank, dtype="float32", extra_dims=extra,
                              elem_dims=elem)
        assert e.data.shape == flat.shape and e.elem_dims == elem


def test_elem_dims_default_is_scalar():
    topo = Topology((1, 1))
    p = Pencil(topo, (4, 5, 6), (1, 2))
    x = PencilArray.empty(p, 0)
    assert x.elem_dims == () and x.ncomp == 1
    assert x.parent_memview().shape == (4, 5, 6)


def test_wrong_flat_length():
    topo = Topology((1, 1))
    p = Pencil(topo, (4, 5, 6), (1, 2))
    with pytest.raises(ValueError, match="incorrect dimensions"):
        PencilArray(p, 0, np.zeros(120), elem_dims=(3,))
    with pytest.raises(ValueError, match="incorrect dimensions"):
        PencilArray(p, 0, np.zeros(360), elem_dims=(2, 2))
    PencilArray(p, 0, np.zeros(360), elem_dims=(3,))


def test_mismatched_elem_dims_raise():
    topo = Topology((1, 1))
    pi = Pencil(topo, (4, 5, 6), (1, 2))
    po = Pencil(topo, (4, 5, 6), (0, 2), permute=(1, 2, 0))
    src = PencilArray.empty(pi, 0, elem_dims=(3,))
    with pytest.raises(ValueError, match="element dimensions"):
        Transposition(PencilArray.empty(po, 0), src)
    with pytest.raises(ValueError, match="element dimensions"):
        Transposition(PencilArray.empty(po, 0, elem_dims=(1, 3)), src)
    with pytest.raises(ValueError, match="element dimensions"):
        run_transpose_sim([PencilArray.empty(po, 0, elem_dims=(2,))], [src])


def test_pencilio_refuses_elem_dims(tmp_path):
    topo = Topology((1, 1))
    p = Pencil(topo, (4, 5, 6), (1, 2))
    x = PencilArray(p, 0, np.zeros(360), elem_dims=(3,))
    f = MPIIOFile(str(tmp_path / "f.bin"), "w")
    with pytest.raises(NotImplementedError, match="elem_dims"):
        f.write("u", x)
    with pytest.raises(NotImplementedError, match="elem_dims"):
        f.read("u", x)
    with pytest.raises(NotImplementedError, match="elem_dims"):
        f.read_raw(x)
    f.close()


# ---- simulated multi-rank transposes vs the C oracle -----------------------

@pytest.mark.parametrize("elem,dtype", ELEMS,
                         ids=lambda v: str(getattr(v, "__name__", v)))
@pytest.mark.parametrize("cfg", SIM_CFGS, ids=_ids)
def test_sim_transpose_matches_c_oracle(cfg, elem, dtype, oracle_lib_path):
    dims, pdims, di, pi, do, po, extra, _ = cfg
    nc = math.prod(elem)
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    g, parents = seeded_elem_parents(dims, pdims, di, pi, extra, dtype, elem)
    nr = topo.nranks
    srcs = [PencilArray(Pi, r, parents[r].copy(), extra, elem)
            for r in range(nr)]
    dsts = [PencilArray.empty(Po, r, dtype=dtype, extra_dims=extra,
                              elem_dims=elem) for r in range(nr)]
    for d in dsts:
        d.data.view(np.uint8)[:] = 0xAB
    run_transpose_sim(dsts, srcs)
    exp = c_oracle_elem(oracle_lib_path, parents, dims, pdims, di, pi, do,
                        po, extra, dtype, nc)
    for r in range(nr):
        assert same_bits(dsts[r].data, exp[r]), f"rank {r}"
        assert same_bits(srcs[r].data, parents[r])  # source untouched

    gs, gd = gather_sim(srcs), gather_sim(dsts)
    assert gs.shape == tuple(elem) + tuple(dims) + tuple(extra)
    assert same_bits(gs, gd)
    assert same_bits(gs, g)


def test_c_oracle_composite_equals_per_component(oracle_lib_path):
    """The reference result used throughout: esz = 24 on interleaved parents
    is three esz = 8 transposes of the separate components."""
    dims, pdims, di, pi, do, po, extra, _ = SWEEP[1]
    g, parents = seeded_elem_parents(dims, pdims, di, pi, extra, np.float64,
                                     (3,))
    exp = c_oracle_elem(oracle_lib_path, parents, dims, pdims, di, pi, do,
                        po, extra, np.float64, 3)
    for c in range(3):
        comp = [p[c::3] for p in parents]
        one = c_oracle_elem(oracle_lib_path, comp, dims, pdims, di, pi, do,
                            po, extra, np.float64, 1)
        for r in range(math.prod(pdims)):
            assert same_bits(exp[r][c::3], one[r])


# ---- world 1: the numpy executor of Transposition.execute ------------------

@pytest.mark.parametrize("elem,dtype", ELEMS,
                         ids=lambda v: str(getattr(v, "__name__", v)))
@pytest.mark.parametrize("perm", [(0, 1, 2), (1, 2, 0), (2, 1, 0)])
def test_world1_numpy_execute(perm, elem, dtype, oracle_lib_path):
    dims = (42, 31, 29)
    nc = math.prod(elem)
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=perm)
    _, parents = seeded_elem_parents(dims, (1, 1), (1, 2), (0, 1, 2), (),
                                     dtype, elem)
    src = PencilArray(Pi, 0, parents[0].copy(), elem_dims=elem)
    dst = PencilArray.empty(Po, 0, dtype=dtype, elem_dims=elem)
    Transposition(dst, src).execute()
    exp = c_oracle_elem(oracle_lib_path, parents, dims, (1, 1), (1, 2),
                        (0, 1, 2), (0, 2), perm, (), dtype, nc)[0]
    assert same_bits(dst.data, exp)


# ---- in place ---------------------------------------------------------------

def test_many_pencil_array_inplace_chain(oracle_lib_path):
    dims, pdims = (16, 21, 41), (1, 1)
    topo = Topology(pdims)
    pens = (
        Pencil(topo, dims, (1, 2)),
        Pencil(topo, dims, (0, 2), permute=(1, 2, 0)),
        Pencil(topo, dims, (0, 1), permute=(2, 1, 0)),
    )
    _, parents = seeded_elem_parents(dims, pdims, (1, 2), (0, 1, 2), (),
                                     np.float64, (3,))
    m = ManyPencilArray(pens, 0, elem_dims=(3,))
    assert all(a.elem_dims == (3,) for a in m.arrays)
    assert m.data.shape == (3 * math.prod(dims),)
    m.first.data[:] = parents[0]
    for a, b in [(0, 1), (1, 2)]:
        t = Transposition(m[b], m[a])
        assert t.aliased
        t.execute()
    exp = c_oracle_elem(oracle_lib_path, parents, dims, pdims, (1, 2),
                        (0, 1, 2), (0, 1), (2, 1, 0), (), np.float64, 3)[0]
    assert same_bits(m[2].data, exp)
    for a, b in [(2, 1), (1, 0)]:
        Transposition(m[b], m[a]).execute()
    assert same_bits(m.first.data, parents[0])


# ---- native plan -------------------------------------------------------------

def _desc_tuple(d):
    if d is None:
        return None
    return (tuple(d.dims), tuple(d.sstrides), d.soffset,
            tuple(d.dstrides), d.doffset)


@pytest.mark.parametrize("cfg", [SWEEP[0], SWEEP[4], SWEEP[9]], ids=_ids)
@pytest.mark.parametrize("aliased", [False, True])
def test_native_plan_ncomp_matches_python(cfg, aliased):
    native = pytest.importorskip("pencilarrays_amd.native")
    if not os.path.exists(native.lib_path()):
        pytest.skip("libpencilhip.so not built")
    dims, pdims, di, pi, do, po, extra, _ = cfg
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    B = 8 * 3
    for rank in range(topo.nranks):
        py = build_plan(Pi, Po, rank, extra, aliased=aliased)
        nat = native.NativePlan(Pi, Po, rank, 8, extra, aliased=aliased,
                                ncomp=3)
        sb, rb = nat.buffer_sizes()
        assert sb == py.send_nelem_total * B
        assert rb == py.recv_nelem_total * B
        assert _desc_tuple(py.local) == nat.copydesc(0)
        assert _desc_tuple(py.self_pack) == nat.copydesc(3)
        assert _desc_tuple(py.self_unpack) == nat.copydesc(4)
        for blk in py.peers:
            info = nat.block_info(blk.peer_k)
            assert (info[4], info[5]) == (blk.send_nelem, blk.recv_nelem)
            assert _desc_tuple(blk.pack) == nat.copydesc(1, blk.peer_k)
            assert _desc_tuple(blk.unpack) == nat.copydesc(2, blk.peer_k)


# ---- gloo, world 2 ------------------------------------------------------------

def _worker(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, repo)
        sys.path.insert(0, os.path.join(repo, "oracle"))
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from elem_util import c_oracle_elem, same_bits, seeded_elem_parents
        from pencilarrays_amd import (
            Pencil, PencilArray, Topology, gather_dist, transpose_into,
        )

        dims, pdims = (16, 21, 41), (2, 1)
        din, pin, dout, pout = (1, 2), (0, 1, 2), (0, 2), (1, 2, 0)
        elem, dtype = (3,), np.float32
        topo = Topology(pdims)
        Pi = Pencil(topo, dims, din, permute=pin)
        Po = Pencil(topo, dims, dout, permute=pout)
        g, parents = seeded_elem_parents(dims, pdims, din, pin, (), dtype,
                                         elem)
        src = PencilArray(Pi, rank, parents[rank].copy(), elem_dims=elem)
        dst = PencilArray.empty(Po, rank, dtype=dtype, elem_dims=elem)
        transpose_into(dst, src)
        lib = os.path.join(repo, "oracle", "liboracle.so")
        exp = c_oracle_elem(lib, parents, dims, pdims, din, pin, dout, pout,
                            (), dtype, 3)
        assert same_bits(dst.data, exp[rank]), f"rank {rank} mismatch"

        gs = gather_dist(src)
        gd = gather_dist(dst)
        if rank == 0:
            assert gs.shape == elem + dims
            assert same_bits(gs, gd) and same_bits(gs, g)

        back = PencilArray.empty(Pi, rank, dtype=dtype, elem_dims=elem)
        transpose_into(back, dst)
        assert same_bits(back.data, parents[rank])
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2_elem_dims(oracle_lib_path):
    mp.spawn(_worker, args=(2, 29433), nprocs=2, join=True)
