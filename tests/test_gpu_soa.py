"""Split and join transposes on one MI355X, bit for bit.

- pa_device_copy_soa in both directions: linear windows at every vector
  width and misalignment, the tile at the tile edges, the generic kernel;
- the stage API as a multi-rank run on ONE GPU, device slice copies at the
  pa_plan_peer_message ranges standing in for the exchange (as in
  test_gpu_many.py), against the C oracle per component, staging against the
  n-field host run on the component copies;
- SplitTransposition / JoinTransposition end to end in world 1;
- launch geometry: a workgroup count past the gridDim.x limit and a window
  past byte 2^32 of the vector-valued side.

Every case asserts the selection through the query with the real pointers
before it launches.  Destinations and staging are 0xAB-filled with 256-byte
guards and whole buffers are compared as bit patterns.
"""

import math

import numpy as np
import pytest

from soa_util import (
    DTYPES, desc_extent, elem_type, interleave, join_case, ref_copy_soa,
    split_case,
)
from pencilarrays_amd import (
    JoinTransposition, Pencil, PencilArray, SplitTransposition, Topology,
    build_plan, run_transpose_sim_many,
)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import (  # noqa: E402
    check_far_sentinel, host_random, max_x, roundup,
)
from pencilarrays_amd import native  # noqa: E402

ID3 = (0, 1, 2)
GUARD = 256
SENT = 0xAB
DEV = "cuda:0"
SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN
LINEAR, TILE, GENERIC = (native.KERNEL_SOA_LINEAR, native.KERNEL_SOA_TILE,
                         native.KERNEL_SOA_GENERIC)
DIRS = pytest.mark.parametrize("direction", [SPLIT, JOIN],
                               ids=["split", "join"])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)


def run_copy(desc, ssz, n, direction, want, seed=1, aos_lead=0,
             field_leads=None):
    """One pa_device_copy_soa.  ``want``: the (kind, V) the query must report
    for the real pointers (V None = any).  ``aos_lead`` / ``field_leads[c]``:
    scalars by which a base pointer sits into its allocation.  Compares every
    destination buffer whole, guard included, with ``ref_copy_soa`` on the
    same random source bytes; returns the query's answer."""
    dims, sstr, soff, dstr, doff = desc
    split = direction == SPLIT
    leads = list(field_leads or [0] * n)
    a_side, f_side = ((sstr, soff), (dstr, doff)) if split else \
        ((dstr, doff), (sstr, soff))
    a_bytes = desc_extent(dims, *a_side) * n * ssz
    f_bytes = desc_extent(dims, *f_side) * ssz
    if split:
        aos_h = host_random(a_bytes, seed)
        fld_h = [np.full(f_bytes + GUARD, SENT, np.uint8) for _ in range(n)]
    else:
        aos_h = np.full(a_bytes + GUARD, SENT, np.uint8)
        fld_h = [host_random(f_bytes, seed + 1 + c) for c in range(n)]
    # device buffers: the same bytes behind `lead` scalars
    aos_all = torch.empty(aos_lead * ssz + aos_h.size, dtype=torch.uint8,
                          device=DEV)
    aos_t = aos_all[aos_lead * ssz:]
    aos_t.copy_(torch.from_numpy(aos_h))
    fld_t = []
    for c in range(n):
        t = torch.empty(leads[c] * ssz + fld_h[c].size, dtype=torch.uint8,
                        device=DEV)[leads[c] * ssz:]
        t.copy_(torch.from_numpy(fld_h[c]))
        fld_t.append(t)
    ref_copy_soa(desc, aos_h, fld_h, ssz, n, split)
    ptrs = [t.data_ptr() for t in fld_t]
    k = native.copy_kernel_kind_soa(desc, ssz, n, direction,
                                    aos_t.data_ptr(), ptrs)
    what = f"ssz={ssz} n={n} dir={direction} {desc} {k}"
    assert k.kind == want[0], what
    if want[1] is not None:
        assert k.vec == want[1], what
    native.device_copy_soa(desc, ssz, n, direction, aos_t.data_ptr(), ptrs)
    torch.cuda.synchronize()
    assert aos_t.cpu().numpy().tobytes() == aos_h.tobytes(), what + " aos"
    for c in range(n):
        assert fld_t[c].cpu().numpy().tobytes() == fld_h[c].tobytes(), \
            what + f" field {c}"
    return k


# ---- linear windows ------------------------------------------------------

# runs of 32 scalars, both sides strided, offsets multiples of 4
LIN = ((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16)
# name: (descriptor, aos lead, field leads, V for 4-byte scalars)
LINEAR_CASES = {
    "full": (LIN, 0, (0, 0, 0), 4),
    "aos_ptr_2": (LIN, 2, (0, 0, 0), 2),
    # a base pointer one scalar into its allocation
    "aos_ptr_1": (LIN, 1, (0, 0, 0), 1),
    "field_ptr_2": (LIN, 0, (0, 2, 0), 2),
    "field_ptr_1": (LIN, 0, (0, 0, 1), 1),
    "soff_2": (((32, 6, 5), (1, 40, 400), 10, (1, 32, 192), 16), 0, (0,) * 3,
               2),
    "doff_1": (((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 17), 0, (0,) * 3,
               1),
    "sstride_2": (((32, 6, 5), (1, 42, 400), 8, (1, 32, 192), 16), 0,
                  (0,) * 3, 2),
    "dstride_1": (((32, 6, 5), (1, 40, 400), 8, (1, 32, 193), 16), 0,
                  (0,) * 3, 1),
    "run_2": (((30, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16), 0, (0,) * 3,
              2),
    "run_1": (((31, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16), 0, (0,) * 3,
              1),
    # more than one workgroup, a ragged last one; 1-D
    "blocks": (((36, 17, 9), (1, 40, 700), 4, (1, 36, 612), 0), 0, (0,) * 3,
               4),
    "one_d": (((1003,), (1,), 3, (1,), 5), 0, (0,) * 3, 1),
}


@DIRS
@pytest.mark.parametrize("case", sorted(LINEAR_CASES))
def test_linear_f32_every_width_and_misalignment(case, direction):
    desc, al, fl, V = LINEAR_CASES[case]
    run_copy(desc, 4, 3, direction, (LINEAR, V), aos_lead=al, field_leads=fl)


@DIRS
@pytest.mark.parametrize("ssz,n,al,fl,V", [
    (8, 2, 0, (0, 0), 2), (8, 3, 0, (0, 0, 0), 2), (8, 4, 0, (0,) * 4, 2),
    (8, 3, 1, (0, 0, 0), 1), (8, 3, 0, (0, 1, 0), 1),
    (4, 2, 0, (0, 0), 4), (4, 4, 0, (0,) * 4, 4), (4, 4, 2, (0,) * 4, 2),
    (16, 2, 0, (0, 0), 1), (16, 3, 0, (0,) * 3, 1), (16, 4, 0, (0,) * 4, 1),
], ids=lambda v: str(v).replace(" ", ""))
def test_linear_other_scalars_and_n(ssz, n, al, fl, V, direction):
    run_copy(LIN, ssz, n, direction, (LINEAR, V), aos_lead=al, field_leads=fl)


# ---- the tile at its edges -----------------------------------------------

def _tile_desc(e0, e1, windowed):
    """(e0, 3, e1): the source side contiguous along axis 0, the destination
    side along axis 2 (``ta`` at position 2), a batch axis of 3 between."""
    if windowed:
        p0, p1 = e0 + 3, e1 + 2
        return ((e0, 3, e1), (1, p0, 3 * p0 + 5), 5,
                (3 * p1 + 7, p1, 1), 3)
    return ((e0, 3, e1), (1, e0, 3 * e0), 0, (3 * e1, e1, 1), 0)


def _tile_shape(ssz, n, direction):
    k = native.copy_kernel_kind_soa(_tile_desc(40, 40, False), ssz, n,
                                    direction)
    assert k.kind == TILE and k.tile_i >= 16 and k.tile_j >= 1
    return k.tile_i, k.tile_j


def _edge_kind(e0, e1, windowed):
    """The kind of ``_tile_desc``: a unit extent drops its axis, and then the
    batch axis is the contiguous one (dense) or none is (windowed)."""
    if e0 > 1 and e1 > 1:
        return TILE
    if windowed:
        return GENERIC
    return LINEAR if e0 == e1 == 1 else TILE


def _edges(T):
    return [1, T - 1, T, T + 1, 2 * T + 1]


@DIRS
@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_tile_f64_at_every_edge(n, windowed, direction):
    ti, tj = _tile_shape(8, n, direction)
    for e0 in _edges(ti):
        for e1 in _edges(tj):
            want = (_edge_kind(e0, e1, windowed), None)
            k = run_copy(_tile_desc(e0, e1, windowed), 8, n, direction, want,
                         seed=e0 * 1000 + e1)
            if k.kind == TILE and e0 > 1 and e1 > 1:
                assert (k.tile_i, k.tile_j) == (ti, tj)


@DIRS
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("ssz", [4, 16])
def test_tile_f32_and_16_byte_corner(ssz, n, direction):
    ti, tj = _tile_shape(ssz, n, direction)
    for e0 in (ti - 1, ti + 1):
        for e1 in (tj - 1, tj + 1):
            for windowed in (False, True):
                run_copy(_tile_desc(e0, e1, windowed), ssz, n, direction,
                         (TILE, 1), seed=e0 * 1000 + e1)


@DIRS
def test_tile_base_one_scalar_into_its_allocation(direction):
    run_copy(_tile_desc(70, 37, True), 8, 3, direction, (TILE, 1), aos_lead=1,
             field_leads=(0, 1, 0))


# ---- the generic kernel ----------------------------------------------------

@DIRS
@pytest.mark.parametrize("ssz,n,desc", [
    (8, 5, LIN),                                   # n = 5, linear
    (8, 5, _tile_desc(37, 21, True)),              # n = 5, permuted
    (16, 5, LIN),                                  # 16 x 5 bytes
    (4, 11, _tile_desc(9, 5, False)),              # more fields than a launch
    (8, 3, ((8, 9), (2, 16), 1, (1, 8), 2)),       # no contiguous source axis
    (8, 3, ((8, 9), (3, 24), 0, (9, 1), 0)),
    # more scalars than one pass of the capped grid has lanes
    (4, 2, ((1500, 1500), (2, 3000), 0, (1500, 1), 0)),
], ids=lambda v: str(v).replace(" ", ""))
def test_generic(ssz, n, desc, direction):
    run_copy(desc, ssz, n, direction, (GENERIC, 1))


def test_empty_descriptor_launches_nothing():
    d = ((0, 4), (1, 8), 0, (1, 8), 0)
    a = _sentinel(64)
    f = [_sentinel(64) for _ in range(3)]
    ptrs = [t.data_ptr() for t in f]
    for direction in (SPLIT, JOIN):
        assert native.copy_kernel_kind_soa(d, 8, 3, direction, a.data_ptr(),
                                           ptrs).kind == native.KERNEL_NONE
        native.device_copy_soa(d, 8, 3, direction, a.data_ptr(), ptrs)
    torch.cuda.synchronize()
    for t in [a] + f:
        assert bool((t == SENT).all())


# ---- the stage API: every rank of a grid on one GPU -----------------------

def _exchange(plans, pyplans, n, sends, recvs):
    """The host's exchange: ONE slice copy per peer pair, all n components."""
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


def _host_staging(cfg, ssz, srcs_c, nbytes_c):
    """send / recv buffers per rank of the n-field HOST run
    (run_transpose_sim_many) on scalar sources ``srcs_c[c][r]``."""
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    n, nr = len(srcs_c), topo.nranks
    dt = DTYPES[ssz]
    srcs = [[PencilArray(Pi, r, srcs_c[c][r].view(dt).copy(), extra)
             for c in range(n)] for r in range(nr)]
    dsts = [[PencilArray(Po, r, np.zeros(nbytes_c[c][r] // ssz, dtype=dt),
                         extra) for c in range(n)] for r in range(nr)]
    out = {}
    run_transpose_sim_many(dsts, srcs, staging_out=out)
    return out


def run_stage_soa(cfg, ssz, n, direction, oracle_lib_path, check=None):
    """All ranks of ``cfg`` on one GPU through the split or join stages and
    the ordinary n-field stages of the other side; asserts destinations ==
    oracle, staging == the n-field host run, guards intact."""
    dims, pdims, di, pi, do, po, extra = cfg
    split = direction == SPLIT
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    if split:
        aos, comps, exp_c = split_case(cfg, ssz, n, oracle_lib_path)
        exp_aos = None
    else:
        comps, exp_c, exp_aos = join_case(cfg, ssz, n, oracle_lib_path)
    ref = _host_staging(cfg, ssz, comps, [[len(x) for x in row]
                                          for row in exp_c])

    pyplans = [build_plan(Pi, Po, r, extra) for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, ssz, extra) for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [_sentinel(s) for s, _ in sizes]
    recvs = [_sentinel(rb) for _, rb in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())

    def up(x):
        return _dev(x) if len(x) else _sentinel(0)

    if split:
        a_t = [up(aos[r]) for r in range(nr)]
        f_t = [[_sentinel(len(exp_c[c][r])) for c in range(n)]
               for r in range(nr)]
    else:
        a_t = [_sentinel(len(exp_aos[r])) for r in range(nr)]
        f_t = [[up(comps[c][r]) for c in range(n)] for r in range(nr)]
    ap = [t.data_ptr() for t in a_t]
    fp = [[t.data_ptr() for t in row] for row in f_t]
    if check is not None:
        for r in range(nr):
            check(plans[r], ap[r], fp[r], sends[r].data_ptr(),
                  recvs[r].data_ptr())

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        if split:
            p.pack_split(n, ap[r], stream)
        else:
            p.pack_many(fp[r], stream)
    _exchange(plans, pyplans, n, sends, recvs)
    for r, p in enumerate(plans):
        if split:
            p.local_split(ap[r], fp[r], stream)
            p.unpack_many(fp[r], stream)
        else:
            p.local_join(fp[r], ap[r], stream)
            p.unpack_join(n, ap[r], stream)
    torch.cuda.synchronize()

    for r in range(nr):
        if split:
            for c in range(n):
                nb = len(exp_c[c][r])
                got = f_t[r][c].cpu().numpy()
                assert got[:nb].tobytes() == exp_c[c][r].tobytes(), (r, c)
                assert (got[nb:] == SENT).all(), f"rank {r} field {c} guard"
        else:
            nb = len(exp_aos[r])
            got = a_t[r].cpu().numpy()
            assert got[:nb].tobytes() == exp_aos[r].tobytes(), r
            assert (got[nb:] == SENT).all(), f"rank {r} guard"
        for side, bufs, i in (("send", sends, 0), ("recv", recvs, 1)):
            got = bufs[r].cpu().numpy()
            nb = sizes[r][i]
            assert got[:nb].tobytes() == ref[side][r].tobytes(), \
                f"rank {r} {side} staging"
            assert (got[nb:] == SENT).all(), f"rank {r} {side} guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)


STAGE_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    # empty ranks: 3 planes over 4 ranks
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ()),
    # extra dims: two more axes behind every descriptor
    ((8, 9, 10), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), (4, 3)),
]


@DIRS
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("ssz", [4, 8, 16], ids=["f32", "f64", "c128"])
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_stage_api_multirank_on_one_gpu(cfg, ssz, n, direction,
                                        oracle_lib_path):
    run_stage_soa(cfg, ssz, n, direction, oracle_lib_path)


@DIRS
def test_slab_with_ragged_tiles_in_every_staged_block(direction,
                                                      oracle_lib_path):
    """x-pencil -> y-pencil of a slab over 2 ranks, permuted output, f64 x 3.
    The local copy of a split and every unpack block of a join run the tile
    with at least two tiles and a ragged last one along BOTH tile axes."""
    n, ssz, P = 3, 8, 2
    ti, tj = _tile_shape(ssz, n, direction)
    dims = (2 * (2 * ti + 3), 2 * (2 * tj + 5), 3)
    seen = []

    def check(p, aos, fields, send, recv):
        # split: the local copy; join: the unpack of every peer block
        if direction == SPLIT:
            cases = [(p.copydesc_many(n, 0, 0), fields)]
        else:
            cases = [(p.copydesc_many(n, 0, 2, k), [recv] * n)
                     for k in range(P)]
        for d, ptrs in cases:
            if d is None:
                continue
            kk = native.copy_kernel_kind_soa(d, ssz, n, direction, aos, ptrs)
            assert kk.kind == TILE, (d, kk)
            ddims, sstr, _, dstr, _ = d
            ta = next(a for a in range(1, len(ddims)) if dstr[a] == 1)
            assert sstr[0] == 1
            assert ddims[0] > ti and ddims[0] % ti
            assert ddims[ta] > tj and ddims[ta] % tj
            seen.append(d)

    cfg = (dims, (P,), (1,), ID3, (0,), (1, 0, 2), ())
    run_stage_soa(cfg, ssz, n, direction, oracle_lib_path, check=check)
    assert len(seen) == (P if direction == SPLIT else P * (P - 1))


# ---- end to end, world 1 ---------------------------------------------------

E2E_DIMS = (130, 67, 35)


def _world1(permuted):
    topo = Topology((1, 1))
    return (Pencil(topo, E2E_DIMS, (1, 2)),
            Pencil(topo, E2E_DIMS, (0, 2),
                   permute=(1, 2, 0) if permuted else None))


def _e2e_cfg(permuted):
    return (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2),
            (1, 2, 0) if permuted else ID3, ())


def _typed(t, ssz):
    return t.view({4: torch.float32, 8: torch.float64,
                   16: torch.complex128}[ssz])


def _guarded(nbytes, ssz):
    """(whole buffer, typed view of its first nbytes)"""
    raw = _sentinel(nbytes)
    return raw, _typed(raw[:nbytes], ssz)


@pytest.mark.parametrize("ssz,n,elem_dims", [(8, 3, (3,)), (4, 4, (2, 2)),
                                             (16, 2, (2,))],
                         ids=["3xf64", "2x2xf32", "2xc128"])
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "perm"])
def test_end_to_end_world1(permuted, ssz, n, elem_dims, oracle_lib_path):
    Pi, Po = _world1(permuted)
    cfg = _e2e_cfg(permuted)
    aos, _, exp = split_case(cfg, ssz, n, oracle_lib_path)
    src = PencilArray(Pi, 0, _typed(_dev(aos[0]), ssz), (), elem_dims)
    raws, dsts = [], []
    for c in range(n):
        raw, v = _guarded(len(exp[c][0]), ssz)
        raws.append(raw)
        dsts.append(PencilArray(Po, 0, v))
    # the selection of the one local copy, with the real pointers
    d = native.NativePlan(Pi, Po, 0, ssz).copydesc_many(n, 0, 0)
    k = native.copy_kernel_kind_soa(d, ssz, n, SPLIT, src.data.data_ptr(),
                                    [x.data.data_ptr() for x in dsts])
    assert k.kind == (TILE if permuted else LINEAR)
    t = SplitTransposition(dsts, src)
    t.execute(sync=False)   # deferred wait
    t.wait()
    for c in range(n):
        got = raws[c].cpu().numpy()
        nb = len(exp[c][0])
        assert got[:nb].tobytes() == exp[c][0].tobytes(), c
        assert (got[nb:] == SENT).all()
    # join the fields back onto the input pencil: the source returns
    raw_b, vb = _guarded(len(aos[0]), ssz)
    back = PencilArray(Pi, 0, vb, (), elem_dims)
    j = JoinTransposition(back, dsts)
    j.execute()
    got = raw_b.cpu().numpy()
    assert got[:len(aos[0])].tobytes() == aos[0].tobytes()
    assert (got[len(aos[0]):] == SENT).all()
    # and a join checked against the oracle on its own
    fields, _, exp_a = join_case(cfg, ssz, n, oracle_lib_path)
    srcs = [PencilArray(Pi, 0, _typed(_dev(fields[c][0]), ssz))
            for c in range(n)]
    raw_d, vd = _guarded(len(exp_a[0]), ssz)
    JoinTransposition(PencilArray(Po, 0, vd, (), elem_dims), srcs).execute()
    got = raw_d.cpu().numpy()
    assert got[:len(exp_a[0])].tobytes() == exp_a[0].tobytes()
    assert (got[len(exp_a[0]):] == SENT).all()


def test_repeated_call_allocates_nothing(oracle_lib_path):
    n, ssz = 3, 8
    Pi, Po = _world1(True)
    aos, _, exp = split_case(_e2e_cfg(True), ssz, n, oracle_lib_path)
    src = PencilArray(Pi, 0, _typed(_dev(aos[0]), ssz), (), (n,))
    dsts = [PencilArray(Po, 0, _typed(_sentinel(len(exp[c][0]))
                                      [:len(exp[c][0])], ssz))
            for c in range(n)]
    back = PencilArray(Pi, 0, _typed(_sentinel(len(aos[0]))[:len(aos[0])],
                                     ssz), (), (n,))
    s, j = SplitTransposition(dsts, src), JoinTransposition(back, dsts)
    s.execute()
    j.execute()
    builds = [x._native.native.stage_table_builds() for x in (s, j)]
    a0 = torch.cuda.memory_allocated()
    c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    s.execute()
    j.execute()
    assert [x._native.native.stage_table_builds() for x in (s, j)] == builds
    assert torch.cuda.memory_allocated() == a0
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == c0
    assert back.data.cpu().numpy().tobytes() == aos[0].tobytes()


# ---- launch geometry --------------------------------------------------------

@DIRS
def test_tile_workgroups_past_the_grid_split(direction):
    """(2, 2, B) with one workgroup per 2 x 2 batch and B past the gridDim.x
    limit of a 256-wide workgroup: the second grid row does real work."""
    ssz, n = 4, 2
    B = max_x(256) + 5
    desc = ((2, 2, B), (1, 2, 4), 0, (2, 1, 4), 0)
    dt = elem_type(ssz)
    split = direction == SPLIT
    rnd = host_random(4 * B * n * ssz, 77).view(dt)
    if split:
        aos_h = rnd                                   # [b][j][i][c]
        fld_h = [np.ascontiguousarray(
            aos_h.reshape(B, 2, 2, n)[..., c].transpose(0, 2, 1)).reshape(-1)
            for c in range(n)]                        # [b][i][j]
    else:
        src = [rnd[c * 4 * B:(c + 1) * 4 * B] for c in range(n)]  # [b][j][i]
        fld_h = src
        aos_h = np.ascontiguousarray(np.stack(
            [s.reshape(B, 2, 2).transpose(0, 2, 1) for s in src],
            axis=-1)).reshape(-1)                     # [b][i][j][c]
    if split:
        a_t = _dev(aos_h.view(np.uint8))
        f_t = [_sentinel(4 * B * ssz) for _ in range(n)]
    else:
        a_t = _sentinel(4 * B * n * ssz)
        f_t = [_dev(np.ascontiguousarray(s).view(np.uint8)) for s in fld_h]
    ptrs = [t.data_ptr() for t in f_t]
    k = native.copy_kernel_kind_soa(desc, ssz, n, direction, a_t.data_ptr(),
                                    ptrs)
    assert k.kind == TILE, k
    wg = math.ceil(2 / k.tile_i) * math.ceil(2 / k.tile_j) * B
    assert wg > max_x(256)
    native.device_copy_soa(desc, ssz, n, direction, a_t.data_ptr(), ptrs)
    torch.cuda.synchronize()
    if split:
        for c in range(n):
            exp = torch.from_numpy(fld_h[c].view(np.uint8)).to(DEV)
            assert torch.equal(f_t[c][:exp.numel()], exp), c
            assert bool((f_t[c][exp.numel():] == SENT).all())
    else:
        exp = torch.from_numpy(aos_h.view(np.uint8)).to(DEV)
        assert torch.equal(a_t[:exp.numel()], exp)
        assert bool((a_t[exp.numel():] == SENT).all())


@DIRS
def test_window_past_2e32_bytes_on_the_vector_side(direction):
    """A (70, 66, 3) permuted window whose offset on the vector-valued side
    lies past byte 2^32: the source of a split, the destination of a join."""
    ssz, n = 8, 3
    dims = (70, 66, 3)
    split = direction == SPLIT
    far_off = roundup((1 << 32) // (n * ssz) + 1, 8)
    if split:   # AoS is the source side: contiguous along axis 0
        a_str, f_str, f_off = (1, 72, 72 * 66 + 8), (68, 1, 68 * 70 + 8), 8
        desc = (dims, a_str, far_off, f_str, f_off)
    else:       # AoS is the destination side: contiguous along axis 1
        a_str, f_str, f_off = (68, 1, 68 * 70 + 8), (1, 72, 72 * 66 + 8), 8
        desc = (dims, f_str, f_off, a_str, far_off)
    span = desc_extent(dims, a_str, 0)            # elements of the window
    assert far_off * n * ssz > 1 << 32
    a_bytes = (far_off + span) * n * ssz
    f_bytes = desc_extent(dims, f_str, f_off) * ssz
    lo = far_off * n * ssz
    huge = torch.empty(a_bytes + GUARD, dtype=torch.uint8, device=DEV)
    try:
        # the host reference works on the window's span alone
        local = (dims, a_str, 0, f_str, f_off) if split else \
            (dims, f_str, f_off, a_str, 0)
        if split:
            win_h = host_random(span * n * ssz, 91)
            fld_h = [np.full(f_bytes + GUARD, SENT, np.uint8)
                     for _ in range(n)]
            huge[lo:lo + win_h.size].copy_(torch.from_numpy(win_h))
        else:
            win_h = np.full(span * n * ssz + GUARD, SENT, np.uint8)
            fld_h = [host_random(f_bytes, 92 + c) for c in range(n)]
            huge.fill_(SENT)
        f_t = [_dev(x) for x in fld_h]
        ref_copy_soa(local, win_h, fld_h, ssz, n, split)
        ptrs = [t.data_ptr() for t in f_t]
        k = native.copy_kernel_kind_soa(desc, ssz, n, direction,
                                        huge.data_ptr(), ptrs)
        assert k.kind == TILE, k
        native.device_copy_soa(desc, ssz, n, direction, huge.data_ptr(), ptrs)
        torch.cuda.synchronize()
        if split:
            for c in range(n):
                assert f_t[c].cpu().numpy().tobytes() == fld_h[c].tobytes(), c
        else:
            got = huge[lo:].cpu().numpy()
            assert got.tobytes() == win_h.tobytes()
            check_far_sentinel(huge, [(lo, huge.numel() - lo)])
    finally:
        huge = None
        torch.cuda.empty_cache()
