"""Grouped converting kernels of a wire plan (PA_PLAN_GROUP_CVT) on one
MI355X: k_group_cvt_linear / k_group_cvt_tile through the stage API as a
multi-rank run, through Transposition / MultiTransposition end to end, and
past the gridDim.x split.

Every case asserts its launch rows through the query with the real pointers
before launching (expected rows: the unflagged plan's rows partitioned by
signature, wire_group_util), prefills destinations and staging with 0xAB behind
256-byte guards, and compares whole buffers as bit patterns with references
that are not the code under test: numpy.astype / torch CPU rounding and the C
oracle on the rounded input."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import assert_split, max_x  # noqa: E402
from pencilarrays_amd import (  # noqa: E402
    ManyPencilArray, MultiTransposition, Pencil, PencilArray, Topology,
    Transposition, native,
)
from test_gpu_wire import E2E_DIMS, STAGE_CFGS  # noqa: E402
from wire_gpu_util import GUARD, SENT, sentinel  # noqa: E402
from wire_group_util import (  # noqa: E402
    GEN, LIN, TILE, expected_of, parents_of, partition,
    run_stage_sim_grouped,
)
from wire_util import (  # noqa: E402
    ELEM_KINDS, PAIRS, ROUND, assert_same, expected_rounded, kind_parents,
    ref_round, seeded_values, specials,
)

ID3 = (0, 1, 2)
PACK, LOCAL, UNPACK = (native.STAGE_PACK, native.STAGE_LOCAL,
                       native.STAGE_UNPACK)


def _rows(l):
    return [(x.kind, x.grouped, x.entries) for x in l]


def _stored(pair):
    return np.dtype(PAIRS[pair][0])


def _seeded(pair):
    return lambda count, seed: seeded_values(count, pair, seed)


# ---- 1. the stage API as a multi-rank run on one GPU ------------------------------

def _kind_case(cfg, kind, n, oracle_lib_path, **kw):
    _, _, pair, nc = ELEM_KINDS[kind]
    dims, pdims, di = cfg[0], cfg[1], cfg[2]
    parents = kind_parents(kind, dims, pdims, di, cfg[6], n, oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)
    st = _stored(pair)
    run_stage_sim_grouped(cfg, pair, nc,
                          [[p.view(st) for p in row] for row in parents],
                          [[e.view(st) for e in row] for row in exp], **kw)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", list(ELEM_KINDS))
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_stage_api_grouped_multirank_on_one_gpu(cfg, kind, n,
                                                oracle_lib_path):
    _kind_case(cfg, kind, n, oracle_lib_path)


def test_stage_api_grouped_aliased(oracle_lib_path):
    """PA_PLAN_ALIASED | PA_PLAN_GROUP_CVT: the staged self block joins the
    grouped rows of the pack and local stages."""
    _kind_case(STAGE_CFGS[0], "f64", 3, oracle_lib_path, aliased=True)


# ---- 2. tile edges inside one group -----------------------------------------------

def _slab(n0, n1, n2, P):
    return ((n0, n1, n2), (P,), (1,), ID3, (0,), (1, 0, 2), ())


def _one_tile_row(r, rows):
    assert [(l.kind, l.grouped) for l in rows[UNPACK]] == [(TILE, True)], \
        (r, rows[UNPACK])
    assert [(l.kind, l.grouped) for l in rows[LOCAL]] == [(TILE, True)], \
        (r, rows[LOCAL])


@pytest.mark.parametrize("pair,nc", [("f64_f32", 1), ("f64_f32", 3),
                                     ("f32_bf16", 1)])
@pytest.mark.parametrize("P", [2, 3])
def test_ragged_tiles_inside_one_group(P, pair, nc, oracle_lib_path):
    """An unpack entry is (my dim-0 range) x (the peer's dim-1 range), tiled
    (128 / ncomp) x 64.  Every entry has two or more tiles along both axes
    and a ragged last tile along axis 0.  P = 2: dim-1 ranges 67 and 68.
    P = 3: ranges 128, 128, 129 -- the ranges of a split differ by at most
    one, so entries of DIFFERENT block counts (2 and 3 tiles along ta) need
    one range on a tile edge; the third ends in a one-wide tile."""
    ti = 128 // nc
    n0 = P * (ti + 3) + 1
    n1 = 135 if P == 2 else 385
    cfg = _slab(n0, n1, 2, P)
    n = 2
    parents = parents_of(cfg, pair, nc, n, _seeded(pair), oracle_lib_path)
    exp = expected_of(cfg, pair, nc, parents, oracle_lib_path)
    seen = set()

    def hook(r, rows):
        _one_tile_row(r, rows)
        assert rows[UNPACK][0].entries == n * (P - 1)
        seen.add(rows[UNPACK][0].workgroups)

    run_stage_sim_grouped(cfg, pair, nc, parents, exp, rows_hook=hook)
    if P == 3:  # ranks see peers of 2+3, 2+3 and 2+2 tiles along ta
        assert len(seen) > 1, seen


def test_tile_extents_one_below_and_above_the_tile(oracle_lib_path):
    """Entries of exactly 1, T - 1 and T + 1 elements along each tile axis
    (T = 128 along axis 0, 64 along ta): two ranks, so each entry is half of
    the global extent.  A unit extent drops out of the descriptor and the
    entry is no tile; the partition says what it is."""
    pair, nc, n = "f64_f32", 1, 2
    for e0 in (1, 127, 129):
        for e1 in (1, 63, 65):
            cfg = _slab(2 * e0, 2 * e1, 3, 2)
            parents = parents_of(cfg, pair, nc, n, _seeded(pair),
                                 oracle_lib_path)
            exp = expected_of(cfg, pair, nc, parents, oracle_lib_path)
            hook = _one_tile_row if e0 > 1 and e1 > 1 else None
            run_stage_sim_grouped(cfg, pair, nc, parents, exp,
                                  rows_hook=hook)


# ---- 3. mixed V in one stage --------------------------------------------------------

def test_one_field_one_scalar_into_its_allocation(oracle_lib_path):
    """Field 1 of 3 starts 8 bytes into its allocations: its packs convert
    one scalar per access, the others two, so the pack stage is two grouped
    linear rows."""
    cfg = STAGE_CFGS[2]
    pair, nc, n = "f64_f32", 1, 3
    parents = parents_of(cfg, pair, nc, n, _seeded(pair), oracle_lib_path)
    exp = expected_of(cfg, pair, nc, parents, oracle_lib_path)

    def hook(r, rows):
        assert _rows(rows[PACK]) == [(LIN, True, 14), (LIN, True, 7)], \
            (r, rows[PACK])
        assert _rows(rows[UNPACK]) == [(TILE, True, 21)], (r, rows[UNPACK])

    run_stage_sim_grouped(cfg, pair, nc, parents, exp, lead={1: 1},
                          rows_hook=hook)


# ---- 4. special values through a grouped stage --------------------------------------

@pytest.mark.parametrize("pair", list(PAIRS))
def test_special_values_through_grouped_stages(pair, oracle_lib_path):
    """Ties, subnormal results, overflow to +-inf, +-0 and NaN, tiled over
    every source: narrowed by the grouped pack, widened by the grouped
    unpack, rounded by the grouped local copy."""
    sp = specials(pair)
    cfg = _slab(20, 22, 5, 2)
    nc, n = 1, 3

    def values(count, seed):
        return np.roll(np.resize(sp, count), seed % len(sp))

    parents = parents_of(cfg, pair, nc, n, values, oracle_lib_path)
    exp = expected_of(cfg, pair, nc, parents, oracle_lib_path)

    def hook(r, rows):
        assert _rows(rows[PACK]) == [(LIN, True, n)]
        assert _rows(rows[LOCAL]) == [(TILE, True, n)]
        assert _rows(rows[UNPACK]) == [(TILE, True, n)]

    run_stage_sim_grouped(cfg, pair, nc, parents, exp, rows_hook=hook)


# ---- 5. ncomp = 5 ---------------------------------------------------------------------

MIX5 = ((9, 16, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ())


@pytest.mark.parametrize("cfg", [MIX5, STAGE_CFGS[2]], ids=["mixed", "slab"])
def test_five_components_generic_beside_grouped(cfg, oracle_lib_path):
    """Five components are past the converting tile.  "mixed": one-plane
    windows without a contiguous axis (generic, one launch each) next to a
    grouped linear row in ONE pack_many call.  "slab": grouped linear packs,
    then transposable unpacks as generic rows."""
    pair, nc, n = "f64_f32", 5, 3
    parents = parents_of(cfg, pair, nc, n, _seeded(pair), oracle_lib_path)
    exp = expected_of(cfg, pair, nc, parents, oracle_lib_path)
    mixed = []

    def hook(r, rows):
        for s in (PACK, LOCAL, UNPACK):
            assert all(l.grouped == (l.kind == LIN) and l.kind in (LIN, GEN)
                       for l in rows[s]), (r, s, rows[s])
        kinds = {l.kind for l in rows[PACK]}
        mixed.append(kinds == {LIN, GEN})
        if cfg is not MIX5:
            assert _rows(rows[UNPACK]) == [(GEN, False, 1)] * 21

    run_stage_sim_grouped(cfg, pair, nc, parents, exp, rows_hook=hook)
    assert any(mixed) == (cfg is MIX5)


# ---- 6. end to end, world 1 -----------------------------------------------------------

def _e2e(kind, po, oracle_lib_path, n=1, lead=None):
    """Sources, 0xAB-prefilled destinations and the expectation of a world-1
    transpose of ``n`` fields; ``lead[f]``: field ``f`` starts that many
    bytes into its allocations."""
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    lead = lead or {}
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2), po, ())
    topo = Topology((1, 1))
    Pi = Pencil(topo, E2E_DIMS, (1, 2))
    Po = Pencil(topo, E2E_DIMS, (0, 2), permute=po)
    parents = kind_parents(kind, E2E_DIMS, (1, 1), (1, 2), (), n,
                           oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)
    tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
    srcs, dsts, raws = [], [], []
    for f in range(n):
        lb, nb = lead.get(f, 0), exp[f][0].nbytes
        s_raw = torch.empty(lb + nb, dtype=torch.uint8, device="cuda:0")
        s_raw[lb:] = torch.from_numpy(
            parents[f][0].copy().view(np.uint8)).to("cuda:0")
        raw = sentinel(lb + nb)
        srcs.append(PencilArray(Pi, 0, s_raw[lb:].view(tdt), elem_dims=elem))
        dsts.append(PencilArray(Po, 0, raw[lb:lb + nb].view(tdt),
                                elem_dims=elem))
        raws.append((raw, lb, nb))
    return PAIRS[pair][1], srcs, dsts, raws, exp


def _check_e2e(dsts, raws, exp):
    torch.cuda.synchronize()
    for f, (d, (raw, lb, nb)) in enumerate(zip(dsts, raws)):
        assert_same(d.data.cpu().numpy(), exp[f][0], f"field {f}")
        assert raw.numel() == lb + nb + GUARD
        assert (raw[:lb] == SENT).all().item(), f"field {f} lead"
        assert (raw[lb + nb:] == SENT).all().item(), f"field {f} guard"


def _local_rows(t, srcs, dsts, grouped=True):
    """The local-stage rows of a (Multi)Transposition's native plan, whose
    native side is made here as its first execute would, and the partition of
    the rows of the same plan without the flag."""
    multi = isinstance(t, MultiTransposition)
    if t._native is None:
        t._native = (native.NativeMultiTransposition if multi
                     else native.NativeTransposition)(t)
    nat = t._native.native
    assert nat.group_cvt() == grouped
    sp = [s.data.data_ptr() for s in srcs]
    dp = [d.data.data_ptr() for d in dsts]
    s0 = srcs[0]
    plain = native.NativePlan(
        s0.pencil, dsts[0].pencil, 0, t.wire.stored.itemsize,
        aliased=t.plan.aliased, ncomp=s0.ncomp * t.wire.comps,
        wire=t.wire.code)
    n = len(srcs)
    per = []
    for f, l in enumerate(plain.stage_launches(n, LOCAL, sp, dp)):
        assert not l.grouped and l.entries == 1
        kk = native.copy_kernel_kind_wire(
            plain.copydesc_many(n, f, 0, 0), t.wire.code, ROUND,
            s0.ncomp * t.wire.comps, sp[f], dp[f])
        assert kk.kind == l.kind
        per.append((l.kind, ROUND, kk.vec, l.workgroups))
    rows = nat.stage_launches(n, LOCAL, sp, dp)
    assert rows == partition(per), (rows, per)
    assert nat.stage_launches(n, PACK, sp, dp) == []
    assert nat.stage_launches(n, UNPACK, sp, dp) == []
    return rows


@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
@pytest.mark.parametrize("kind", ["f64", "c128", "3xf64", "f32_bf16"])
def test_world1_transposition_grouped(kind, po, oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e(kind, po, oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], wire_dtype=wname, wire_grouped=True)
    rows = _local_rows(t, srcs, dsts)
    assert _rows(rows) == [(LIN if po == ID3 else TILE, True, 1)]
    t.execute()
    nat = t._native.native
    assert nat.plan_wire() == PAIRS[ELEM_KINDS[kind][2]][2]
    _check_e2e(dsts, raws, exp)
    # a repeated call reuses the stage table
    builds = nat.stage_table_builds()
    assert builds >= 1
    t.execute()
    assert nat.stage_table_builds() == builds
    _check_e2e(dsts, raws, exp)


def test_world1_grouped_async_then_wait(oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], wire_dtype=torch.float32,
                      wire_grouped=True)
    _local_rows(t, srcs, dsts)
    t.execute(sync=False)
    t.wait()
    _check_e2e(dsts, raws, exp)


@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
def test_world1_multitransposition_one_field_8_bytes_off(po, oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e("f64", po, oracle_lib_path, n=3,
                                        lead={1: 8})
    mt = MultiTransposition(dsts, srcs, wire_dtype=wname, wire_grouped=True)
    rows = _local_rows(mt, srcs, dsts)
    if po == ID3:  # the field 8 bytes off converts one scalar per access
        assert _rows(rows) == [(LIN, True, 2), (LIN, True, 1)]
    else:
        assert _rows(rows) == [(TILE, True, 3)]
    mt.execute()
    _check_e2e(dsts, raws, exp)
    nat = mt._native.native
    builds = nat.stage_table_builds()
    mt.execute()
    assert nat.stage_table_builds() == builds
    _check_e2e(dsts, raws, exp)


def test_world1_grouped_inplace_round_trip(oracle_lib_path):
    """x -> y -> x in place over a ManyPencilArray returns round_w(src)."""
    topo = Topology((1, 1))
    pens = (Pencil(topo, E2E_DIMS, (1, 2)),
            Pencil(topo, E2E_DIMS, (0, 2), permute=(1, 2, 0)))
    src = kind_parents("f64", E2E_DIMS, (1, 1), (1, 2), (), 1,
                       oracle_lib_path)[0][0]
    m = ManyPencilArray(pens, 0, device="cuda:0")
    m[0].data.copy_(torch.from_numpy(src))
    fwd = Transposition(m[1], m[0], wire_dtype="float32", wire_grouped=True)
    assert fwd.aliased
    fwd._native = native.NativeTransposition(fwd)
    nat = fwd._native.native
    assert nat.group_cvt()
    sp, dp = [m[0].data.data_ptr()], [m[1].data.data_ptr()]
    assert _rows(nat.stage_launches(1, PACK, sp, dp)) == [(LIN, True, 1)]
    assert _rows(nat.stage_launches(1, LOCAL, sp, dp)) == [(TILE, True, 1)]
    fwd.execute()
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    exp = expected_rounded("f64", [[src]], cfg, oracle_lib_path)[0][0]
    assert_same(m[1].data.cpu().numpy(), exp, "forward")
    Transposition(m[0], m[1], wire_dtype="float32",
                  wire_grouped=True).execute()
    assert_same(m[0].data.cpu().numpy(), ref_round(src, "f64_f32"), "back")


def test_grouped_execute_without_set_buffers(oracle_lib_path):
    """An aliased world-1 plan stages its self block; with no
    pa_plan_set_buffers pa_transpose_execute allocates that staging itself,
    in wire bytes, and the n = 1 stage path it runs accepts it."""
    wname, srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), oracle_lib_path)
    s, d = srcs[0], dsts[0]
    p = native.NativePlan(s.pencil, d.pencil, 0, 8, aliased=True,
                          wire=native.WIRE_F64_F32, group_cvt=True)
    assert p.group_cvt()
    assert p.buffer_sizes() == (0, 4 * len(s))
    sp, dp = [s.data.data_ptr()], [d.data.data_ptr()]
    assert _rows(p.stage_launches(1, PACK, sp, dp)) == [(LIN, True, 1)]
    assert _rows(p.stage_launches(1, LOCAL, sp, dp)) == [(TILE, True, 1)]
    p.execute(sp[0], dp[0], 0)
    p.wait(0)
    _check_e2e(dsts, raws, exp)
    # two fields do not fit the engine's own single-field staging
    with pytest.raises(RuntimeError, match="pa_plan_set_buffers"):
        p.execute_many(sp * 2, dp * 2, 0)


# ---- 7. grouped CVT_TILE past the gridDim.x split -------------------------------------

@pytest.mark.parametrize("kind", ["f64", "f32_bf16"])
def test_grouped_cvt_tile_past_the_split(kind, oracle_lib_path):
    """Three fields, x-pencil to y-pencil with permute (1, 0, 2): the batch
    axis cannot merge with the transposed pair, so the local stage is one
    grouped converting tile launch of three entries of 1398103 one-tile
    batches each: 4194309 workgroups of 1024 threads against a gridDim.x
    limit of 4194303, the grid-row boundary strictly inside the third
    entry."""
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    dims, n, wg, threads = (2, 2, 1398103), 3, 4194309, 1024
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 0, 2))
    cfg = (dims, (1, 1), (1, 2), ID3, (0, 2), (1, 0, 2), ())
    parents = kind_parents(kind, dims, (1, 1), (1, 2), (), n,
                           oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)
    isz = _stored(pair).itemsize
    plan = native.NativePlan(Pi, Po, 0, isz, wire=PAIRS[pair][2],
                             group_cvt=True)
    plain = native.NativePlan(Pi, Po, 0, isz, wire=PAIRS[pair][2])
    srcs = [torch.from_numpy(parents[f][0].view(np.uint8)).to("cuda:0")
            for f in range(n)]
    dsts = [sentinel(exp[f][0].nbytes) for f in range(n)]
    sp = [t.data_ptr() for t in srcs]
    dp = [t.data_ptr() for t in dsts]
    try:
        rows = plan.stage_launches(n, LOCAL, sp, dp)
        assert [tuple(l) for l in rows] == [(TILE, True, 3, wg)], rows
        unflagged = plain.stage_launches(n, LOCAL, sp, dp)
        assert [tuple(l) for l in unflagged] == \
            [(TILE, False, 1, wg // 3)] * 3
        assert_split(wg, threads)
        per = wg // 3
        assert 3 * per == wg and 2 * per < max_x(threads) < wg - 1
        assert plan.stage_launches(n, PACK, sp, dp) == []
        assert plan.stage_launches(n, UNPACK, sp, dp) == []
        plan.execute_many(sp, dp, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for f in range(n):
            got = dsts[f].cpu().numpy()
            nb = exp[f][0].nbytes
            assert (got[nb:] == SENT).all(), f"field {f} guard"
            assert_same(got[:nb].view(dtype), exp[f][0], f"field {f}")
    finally:
        del srcs, dsts, plan, plain
        torch.cuda.empty_cache()
