"""Multi-field transposes on one MI355X, bit-exact against the C oracle.

- the stage API as a multi-rank run on ONE GPU: one native plan per simulated
  rank, pa_transpose_pack_many -> device slice copies at the
  pa_plan_peer_message ranges (standing in for the host's exchange) ->
  pa_transpose_local_many -> pa_transpose_unpack_many.  This runs the P > 1
  pack / staging-offset / unpack body of the engine on a GPU;
- tile edges inside one grouped launch;
- n = 1 grouped execution vs pa_transpose_execute, byte for byte;
- MultiTransposition end to end, table-cache lifetime, no steady-state
  allocation.

Destinations and staging buffers are prefilled with a sentinel and carry a
guard tail; whole buffers are compared, so out-of-window writes are caught.
"""

import math

import numpy as np
import pytest

from many_util import expected_dests, random_parents
from pencilarrays_amd import (
    MultiTransposition, Pencil, PencilArray, Topology, build_plan,
)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402

ID3 = (0, 1, 2)
GUARD = 256   # guard bytes behind every destination and staging buffer
SENT = 0xAB


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8,
                      device="cuda:0")


def _guard_ok(t, nbytes):
    return bool((t[nbytes:] == SENT).all().item())


def run_stage_sim(cfg, ssz, ncomp, n, oracle_lib_path, check_launches=None):
    """All ranks of `cfg` on one GPU through the stage API; returns nothing,
    asserts destinations == oracle and guards intact."""
    dims, pdims, di, pi, do, po, extra = cfg
    esz = ssz * ncomp
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    parents = random_parents(dims, pdims, di, extra, esz, n, oracle_lib_path)
    exp = expected_dests(parents, cfg, esz, oracle_lib_path)

    pyplans = [build_plan(Pi, Po, r, extra) for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, ssz, extra, ncomp=ncomp)
             for r in range(nr)]
    srcs = [[_dev(parents[f][r]) if len(parents[f][r]) else _sentinel(0)
             for f in range(n)] for r in range(nr)]
    dsts = [[_sentinel(len(exp[f][r])) for f in range(n)] for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [_sentinel(s) for s, _ in sizes]
    recvs = [_sentinel(rb) for _, rb in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
    sp = [[t.data_ptr() for t in srcs[r]] for r in range(nr)]
    dp = [[t.data_ptr() for t in dsts[r]] for r in range(nr)]
    if check_launches is not None:
        for r, p in enumerate(plans):
            check_launches(p, pyplans[r], sp[r], dp[r])

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        p.pack_many(sp[r], stream)
    # the host's exchange: ONE slice copy per peer pair, all n fields in it
    for r, p in enumerate(plans):
        for blk in pyplans[r].peers:
            if blk.peer_k == pyplans[r].my_k:
                continue
            so, sn, _, _ = p.peer_message(n, blk.peer_k)
            _, _, ro, rn = plans[blk.global_rank].peer_message(
                n, pyplans[r].my_k)
            assert sn == rn
            if sn:
                recvs[blk.global_rank][ro:ro + rn] = sends[r][so:so + sn]
    for r, p in enumerate(plans):
        p.local_many(sp[r], dp[r], stream)
        p.unpack_many(dp[r], stream)
    torch.cuda.synchronize()

    for r in range(nr):
        for f in range(n):
            nb = len(exp[f][r])
            got = dsts[r][f].cpu().numpy()
            assert got[:nb].tobytes() == exp[f][r].tobytes(), \
                f"rank {r} field {f}"
            assert (got[nb:] == SENT).all(), f"rank {r} field {f} guard"
        assert _guard_ok(sends[r], sizes[r][0]), f"rank {r} send guard"
        assert _guard_ok(recvs[r], sizes[r][1]), f"rank {r} recv guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)


# the reference chain dims: uneven splits, so entries differ in block count
STAGE_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    # empty ranks: 3 planes over 4 ranks
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ()),
]
# f64, f32, int16, complex128, elem_dims=(3,) of f32
ELEMS = [(8, 1), (4, 1), (2, 1), (16, 1), (4, 3)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ssz,ncomp", ELEMS,
                         ids=["f64", "f32", "i16", "c128", "3xf32"])
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_stage_api_multirank_on_one_gpu(cfg, ssz, ncomp, n, oracle_lib_path):
    run_stage_sim(cfg, ssz, ncomp, n, oracle_lib_path)


# x-pencil -> y-pencil of a slab, permuted output.  On rank r the unpack
# entry of peer k moves (local dim 0) x (peer k's share of dim 1) x dim 2:
# axis 0 is tiled by TI and dim 1 (the destination-contiguous axis) by TJ.
# Every entry has >= 2 tiles along both axes and a ragged last tile along
# axis 0.  The shares of dim 1 differ by at most one, so entries of ONE
# launch can differ in block count only where a share is a whole number of
# tiles:
# - odd extents (TILE, 128 x 64): shares of 128 and 129, i.e. 2 full tiles
#   next to 2 full tiles plus a ragged one-wide tile — entries of one launch
#   differ in block count;
# - even extents (TILE_VS, 64 x 128): every share must start on an even index
#   to keep 16-byte stores, so all shares are equal; every entry is ragged
#   along both axes and entries of one launch have equal counts.
EDGE_CFGS = [
    # (dims, P, kind, TI, TJ)
    ((260, 264, 4), 2, "TILE_VS", 64, 128),
    ((394, 780, 4), 3, "TILE_VS", 64, 128),
    ((261, 257, 3), 2, "TILE", 128, 64),
    ((393, 385, 3), 3, "TILE", 128, 64),
]


@pytest.mark.parametrize("dims,P,kind,TI,TJ", EDGE_CFGS,
                         ids=lambda v: str(v).replace(" ", ""))
def test_tile_edges_inside_a_group(dims, P, kind, TI, TJ, oracle_lib_path):
    n = 3
    want = {"TILE": native.KERNEL_TILE, "TILE_VS": native.KERNEL_TILE_VS}[kind]
    counts, ragged_ta = set(), set()

    def check(p, pyp, sp, dp):
        for stage, entries in ((native.STAGE_UNPACK, (P - 1) * n),
                               (native.STAGE_LOCAL, n)):
            rows = p.stage_launches(n, stage, sp, dp)
            assert [(l.kind, l.grouped, l.entries) for l in rows] == \
                [(want, True, entries)], (stage, rows)
        for k in range(P):
            d = p.copydesc_many(n, 0, 2, k)
            if d is None:
                continue
            ddims, sstr, _, dstr, _ = d
            ta = next(a for a in range(1, len(ddims)) if dstr[a] == 1)
            assert sstr[0] == 1
            assert ddims[0] > TI and ddims[0] % TI
            assert ddims[ta] > TJ
            ragged_ta.add(ddims[ta] % TJ != 0)
            counts.add(math.ceil(ddims[0] / TI) * math.ceil(ddims[ta] / TJ))

    cfg = (dims, (P,), (1,), ID3, (0,), (1, 0, 2), ())
    run_stage_sim(cfg, 8, 1, n, oracle_lib_path, check_launches=check)
    assert True in ragged_ta
    if kind == "TILE":
        assert len(counts) > 1, "entries should differ in block count"
    else:
        assert ragged_ta == {True}


WORLD1 = [
    # identity, permuted, extra dims
    ((42, 31, 29), (1, 2), ID3, (0, 2), ID3, ()),
    ((64, 64, 64), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((42, 31, 29), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((24, 18, 12), (1, 2), ID3, (0, 2), (1, 2, 0), (4, 3)),
]


@pytest.mark.parametrize("cfg", WORLD1,
                         ids=lambda c: f"{c[0]}_p{c[4]}_e{c[5]}")
def test_n1_grouped_equals_execute(cfg):
    dims, di, pi, do, po, extra = cfg
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nbytes = Pi.length_local(0) * math.prod(extra or (1,)) * 8
    rng = np.random.default_rng(7)
    src = _dev(rng.integers(0, 256, nbytes, dtype=np.uint8))
    one, many = _sentinel(nbytes), _sentinel(nbytes)
    p1 = native.NativePlan(Pi, Po, 0, 8, extra)
    p1.execute(src.data_ptr(), one.data_ptr(), 0)
    p2 = native.NativePlan(Pi, Po, 0, 8, extra)
    rows = p2.stage_launches(1, native.STAGE_LOCAL, [src.data_ptr()],
                             [many.data_ptr()])
    assert len(rows) == 1 and rows[0].grouped
    p2.execute_many([src.data_ptr()], [many.data_ptr()], 0)
    torch.cuda.synchronize()
    assert torch.equal(one, many)
    assert _guard_ok(many, nbytes)
    assert not torch.equal(many[:nbytes], torch.full_like(many[:nbytes], SENT))


def _world1_pencils(dims=(64, 48, 40)):
    topo = Topology((1, 1))
    return (Pencil(topo, dims, (1, 2)),
            Pencil(topo, dims, (0, 2), permute=(1, 2, 0)))


def _oracle_world1(src_bytes, dims, oracle_lib_path):
    cfg = (dims, (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    return expected_dests([[src_bytes]], cfg, 8, oracle_lib_path)[0][0]


def test_multitransposition_world1_odd_offset_field(oracle_lib_path):
    """Three f64 fields; field 1 lives 8 bytes into its allocations, so its
    destination loses the 16-byte alignment the others have and its entries
    run the scalar tile next to the others' vector-store tile."""
    dims = (64, 48, 40)
    Pi, Po = _world1_pencils(dims)
    L = Pi.length_local(0)
    rng = np.random.default_rng(21)
    src_np = [rng.standard_normal(L) for _ in range(3)]
    srcs, dsts, raw = [], [], []
    for f in range(3):
        lead = 1 if f == 1 else 0
        s = torch.empty(L + lead, dtype=torch.float64, device="cuda:0")[lead:]
        s.copy_(torch.from_numpy(src_np[f]))
        d_all = torch.full((L + lead + 32,), float("nan"),
                           dtype=torch.float64, device="cuda:0")
        raw.append(d_all)
        srcs.append(PencilArray(Pi, 0, s))
        dsts.append(PencilArray(Po, 0, d_all[lead:lead + L]))
    assert dsts[1].data.data_ptr() % 16 == 8
    mt = MultiTransposition([d for d in dsts], srcs)
    assert not mt.aliased
    mt.execute()
    rows = mt._native.native.stage_launches(
        3, native.STAGE_LOCAL, [s.data.data_ptr() for s in srcs],
        [d.data.data_ptr() for d in dsts])
    assert sorted((l.kind, l.grouped, l.entries) for l in rows) == \
        [(native.KERNEL_TILE, True, 1), (native.KERNEL_TILE_VS, True, 2)]
    for f in range(3):
        exp = _oracle_world1(src_np[f].view(np.uint8), dims, oracle_lib_path)
        got = dsts[f].data.cpu().numpy()
        assert got.view(np.uint8).tobytes() == exp.tobytes(), f
        lead = 1 if f == 1 else 0
        tail = raw[f].cpu().numpy()
        assert np.isnan(tail[:lead]).all() and np.isnan(tail[lead + L:]).all()


def test_multitransposition_inplace_round_trip(oracle_lib_path):
    """x -> y -> x over aliased pairs: every field transposed in place."""
    dims = (64, 48, 40)
    Pi, Po = _world1_pencils(dims)
    L = Pi.length_local(0)
    assert Po.length_local(0) == L
    rng = np.random.default_rng(22)
    src_np = [rng.standard_normal(L) for _ in range(2)]
    bufs = [_dev(a) for a in src_np]
    xs = [PencilArray(Pi, 0, b) for b in bufs]
    ys = [PencilArray(Po, 0, b) for b in bufs]
    fwd = MultiTransposition(ys, xs)
    assert fwd.aliased and fwd.plan.aliased
    fwd.execute()
    for f in range(2):
        exp = _oracle_world1(src_np[f].view(np.uint8), dims, oracle_lib_path)
        assert bufs[f].cpu().numpy().view(np.uint8).tobytes() == exp.tobytes()
    MultiTransposition(xs, ys).execute()
    for f in range(2):
        assert np.array_equal(bufs[f].cpu().numpy(), src_np[f])


def test_back_to_back_async_calls_and_steady_state(oracle_lib_path):
    """Two execute(sync=False) on different array sets, then wait(): both
    correct (each set has its own table; neither is rewritten while the
    other's launches are in flight).  Then a repeated call builds and
    allocates nothing."""
    dims = (64, 48, 40)
    Pi, Po = _world1_pencils(dims)
    L = Pi.length_local(0)
    rng = np.random.default_rng(23)
    n = 3
    sets = []
    for _ in range(2):
        src_np = [rng.standard_normal(L) for _ in range(n)]
        srcs = [PencilArray(Pi, 0, _dev(a)) for a in src_np]
        dsts = [PencilArray(Po, 0, torch.full((L,), float("nan"),
                                              dtype=torch.float64,
                                              device="cuda:0"))
                for _ in range(n)]
        sets.append((src_np, srcs, dsts))
    mt = MultiTransposition(sets[0][2], sets[0][1])
    mt.execute(sync=False)
    # same plan object, other arrays: re-point the executor's array set
    mt.srcs, mt.dests = sets[1][1], sets[1][2]
    mt.execute(sync=False)
    mt.wait()
    torch.cuda.synchronize()
    for src_np, _, dsts in sets:
        for f in range(n):
            exp = _oracle_world1(src_np[f].view(np.uint8), dims,
                                 oracle_lib_path)
            assert dsts[f].data.cpu().numpy().view(np.uint8).tobytes() == \
                exp.tobytes()

    nat = mt._native.native
    tables = nat.stage_table_count()
    assert tables >= 2  # one local-stage table per array set at least
    pool = mt._native._pool
    v0 = pool.version if pool is not None else None
    a0 = torch.cuda.memory_allocated()
    c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    mt.execute()
    mt.srcs, mt.dests = sets[0][1], sets[0][2]
    mt.execute()
    assert nat.stage_table_count() == tables, "steady state built a table"
    assert torch.cuda.memory_allocated() == a0
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == c0
    if pool is not None:
        assert pool.version == v0
