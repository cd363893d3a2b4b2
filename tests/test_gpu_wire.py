"""Reduced-precision wire on one MI355X: the converting kernels through
pa_device_copy_wire, the stage API as a multi-rank run, and Transposition /
MultiTransposition end to end — all against references that are not the code
under test (numpy.astype, torch CPU bfloat16, the C oracle on the rounded
input), compared as bit patterns.

Every device case asserts the kernel selection through the query with the
real pointers first; destinations and staging buffers are prefilled with
0xAB and carry a 256-byte guard; whole buffers are compared."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import (  # noqa: E402
    ManyPencilArray, MultiTransposition, Pencil, PencilArray, Topology,
    Transposition, native,
)
from wire_gpu_util import (  # noqa: E402
    SENT, dev, run_copy, run_stage_sim, sentinel, side_types, transpose_desc,
)
from wire_util import (  # noqa: E402
    ELEM_KINDS, NARROW, PAIRS, ROUND, WIDEN, assert_same, expected_rounded,
    kind_parents, ref_round,
)

LIN, TILE, GEN = (native.KERNEL_CVT_LINEAR, native.KERNEL_CVT_TILE,
                  native.KERNEL_CVT_GENERIC)
OPS = [NARROW, WIDEN, ROUND]
OP_IDS = ["narrow", "widen", "round"]
ID3 = (0, 1, 2)
NB = 3


def _full_v(pair, op):
    s, d = side_types(pair, op)
    return 16 // max(s.itemsize, d.itemsize)


# ---- pa_device_copy_wire: linear ---------------------------------------------

@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_special_values_through_1d_copy(pair, op):
    """Every special value (ties, subnormal results, overflow, +-0, +-inf,
    NaN) sits in the first 110 scalars of the seeded input."""
    for n in (128, 1000):
        run_copy(((n,), (1,), 0, (1,), 0), pair, op, 1, 7, LIN,
                 _full_v(pair, op))
    # two and three components: the run is dims[0] * ncomp scalars
    run_copy(((126,), (1,), 0, (1,), 0), pair, op, 2, 8, LIN,
             _full_v(pair, op))
    run_copy(((43,), (1,), 0, (1,), 0), pair, op, 3, 9, LIN, 1)


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_linear_windows_at_each_vector_width(pair, op):
    V = _full_v(pair, op)
    h = V // 2
    # dims, sstr, soff, dstr, doff: every quantity a multiple of 4
    base = ((24, 5, 3), (1, 32, 200), 8, (1, 28, 140), 4)
    run_copy(base, pair, op, 1, 11, LIN, V)
    # one misalignment at a time lowers V to what it still allows
    run_copy(base, pair, op, 1, 12, LIN, h, src_lead=h)
    run_copy(base, pair, op, 1, 13, LIN, h, dst_lead=h)
    run_copy(base, pair, op, 1, 14, LIN, 1, src_lead=1)
    run_copy(base, pair, op, 1, 15, LIN, 1, dst_lead=3)
    run_copy(((24, 5, 3), (1, 32, 200), 8 + h, (1, 28, 140), 4), pair, op, 1,
             16, LIN, h)
    run_copy(((24, 5, 3), (1, 32, 200), 8, (1, 28, 140), 4 + 1), pair, op, 1,
             17, LIN, 1)
    run_copy(((24, 5, 3), (1, 32 + h, 200), 8, (1, 28, 140), 4), pair, op, 1,
             18, LIN, h)
    run_copy(((24, 5, 3), (1, 32, 200), 8, (1, 28, 140 + 1), 4), pair, op, 1,
             19, LIN, 1)
    run_copy(((24 + h, 5, 3), (1, 32, 200), 8, (1, 28, 140), 4), pair, op, 1,
             20, LIN, h)
    run_copy(((23, 5, 3), (1, 32, 200), 8, (1, 28, 140), 4), pair, op, 1,
             21, LIN, 1)
    # more than one workgroup, three components
    run_copy(((100, 9, 3), (1, 104, 1000), 4, (1, 100, 900), 0), pair, op, 3,
             22, LIN, V)


# ---- pa_device_copy_wire: tile -------------------------------------------------

def _tile_dims(pair, op, nc):
    k = native.copy_kernel_kind_wire(
        ((40, 50, 3), (1, 40, 2000), 0, (50, 1, 2000), 0), PAIRS[pair][2],
        op, nc, 4096, 4096)
    assert k.kind == TILE and k.tile_i > 0 and k.tile_j > 0
    return k.tile_i, k.tile_j


def _edges(t):
    return [1, t - 1, t, t + 1, 2 * t + 1]


def _tile_case(pair, op, nc, n0, nta, layout, seed, **lead):
    dense = layout == "dense"
    ta_pos = 2 if layout == "window_ta2" else 1
    sp, so, dp, do = (n0, 0, nta, 0) if dense else (n0 + 5, 3, nta + 3, 2)
    desc = transpose_desc(n0, nta, NB, sp, so, dp, do, ta_pos)
    if n0 > 1 and nta > 1:
        want = TILE
    else:
        # a unit extent drops out of the normalized descriptor: dense
        # buffers merge into one run, a window keeps no axis that is
        # unit-stride on both sides
        want = LIN if dense else GEN
    return run_copy(desc, pair, op, nc, seed, want, **lead)


@pytest.mark.parametrize("layout", ["dense", "window", "window_ta2"])
@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("nc", [1, 2, 3])
def test_tile_boundary_sweep_f64_f32(nc, op, layout):
    """5 x 5 extents around the tile edges on both tile axes, batch 3."""
    ti, tj = _tile_dims("f64_f32", op, nc)
    seed = 100
    for n0 in _edges(ti):
        for nta in _edges(tj):
            seed += 1
            _tile_case("f64_f32", op, nc, n0, nta, layout, seed)


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("pair", ["f32_f16", "f32_bf16"])
def test_tile_corner_f32_pairs(pair, nc, op):
    ti, tj = _tile_dims(pair, op, nc)
    seed = 200
    for n0 in (ti - 1, ti + 1):
        for nta in (tj - 1, tj + 1):
            for layout in ("window", "window_ta2"):
                seed += 1
                _tile_case(pair, op, nc, n0, nta, layout, seed)


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_tile_base_pointer_one_scalar_into_allocation(pair, op):
    ti, tj = _tile_dims(pair, op, 1)
    _tile_case(pair, op, 1, ti + 1, tj + 1, "window", 300, src_lead=1,
               dst_lead=1)
    _tile_case(pair, op, 2, ti + 1, tj - 1, "dense", 301, src_lead=1,
               dst_lead=1)


# ---- pa_device_copy_wire: generic ------------------------------------------------

@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_generic_fallback(pair, op):
    # no axis contiguous on the source
    run_copy(((7, 5), (2, 20), 1, (3, 40), 2), pair, op, 1, 400, GEN, 1)
    run_copy(((7, 5), (2, 20), 1, (3, 40), 2), pair, op, 2, 401, GEN, 1)
    # transposable, but five components are past the tile
    run_copy(transpose_desc(70, 66, NB, 75, 3, 69, 2), pair, op, 5, 402, GEN,
             1)


# ---- the stage API as a multi-rank run on one GPU ----------------------------------

STAGE_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    # empty ranks: 3 planes over 4 ranks
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ()),
]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", list(ELEM_KINDS))
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_stage_api_multirank_on_one_gpu(cfg, kind, n, oracle_lib_path):
    run_stage_sim(cfg, kind, n, oracle_lib_path)


@pytest.mark.parametrize("kind", ["f64", "f32_bf16"])
def test_stage_api_aliased(kind, oracle_lib_path):
    """PA_PLAN_ALIASED: the self block is narrowed into the recv tail by the
    pack stage and widened out of it by the local stage."""
    run_stage_sim(STAGE_CFGS[0], kind, 3, oracle_lib_path, aliased=True)


# ---- end to end, world 1 --------------------------------------------------------------

E2E_DIMS = (130, 67, 35)


def _e2e(kind, po, oracle_lib_path, n=1):
    dtype, elem, pair, nc = ELEM_KINDS[kind]
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
        s = torch.from_numpy(parents[f][0].copy()).to("cuda:0")
        raw = sentinel(exp[f][0].nbytes)
        d = raw[:exp[f][0].nbytes].view(tdt)
        srcs.append(PencilArray(Pi, 0, s, elem_dims=elem))
        dsts.append(PencilArray(Po, 0, d, elem_dims=elem))
        raws.append(raw)
    return PAIRS[pair][1], srcs, dsts, raws, exp


def _check_e2e(dsts, raws, exp):
    torch.cuda.synchronize()
    for f, (d, raw) in enumerate(zip(dsts, raws)):
        assert_same(d.data.cpu().numpy(), exp[f][0], f"field {f}")
        assert (raw[exp[f][0].nbytes:] == SENT).all().item()


@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
@pytest.mark.parametrize("kind", ["f64", "c128", "3xf64", "f32_bf16"])
def test_world1_transposition(kind, po, oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e(kind, po, oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], wire_dtype=wname)
    t.execute()
    nat = t._native.native
    assert nat.plan_wire() == PAIRS[ELEM_KINDS[kind][2]][2]
    rows = nat.stage_launches(1, native.STAGE_LOCAL,
                              [srcs[0].data.data_ptr()],
                              [dsts[0].data.data_ptr()])
    assert [l.kind for l in rows] == [LIN if po == ID3 else TILE]
    _check_e2e(dsts, raws, exp)


def test_world1_async_then_wait(oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], wire_dtype=torch.float32)
    t.execute(sync=False)
    t.wait()
    _check_e2e(dsts, raws, exp)


def test_world1_multitransposition_three_fields(oracle_lib_path):
    wname, srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), oracle_lib_path,
                                        n=3)
    mt = MultiTransposition(dsts, srcs, wire_dtype=wname)
    mt.execute()
    rows = mt._native.native.stage_launches(
        3, native.STAGE_LOCAL, [s.data.data_ptr() for s in srcs],
        [d.data.data_ptr() for d in dsts])
    assert [(l.kind, l.grouped) for l in rows] == [(TILE, False)] * 3
    _check_e2e(dsts, raws, exp)


def test_world1_inplace_round_trip(oracle_lib_path):
    """x -> y -> x in place over a ManyPencilArray returns round_w(src)."""
    topo = Topology((1, 1))
    pens = (Pencil(topo, E2E_DIMS, (1, 2)),
            Pencil(topo, E2E_DIMS, (0, 2), permute=(1, 2, 0)))
    src = kind_parents("f64", E2E_DIMS, (1, 1), (1, 2), (), 1,
                       oracle_lib_path)[0][0]
    m = ManyPencilArray(pens, 0, device="cuda:0")
    m[0].data.copy_(torch.from_numpy(src))
    fwd = Transposition(m[1], m[0], wire_dtype="float32")
    assert fwd.aliased
    fwd.execute()
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    exp = expected_rounded("f64", [[src]], cfg, oracle_lib_path)[0][0]
    assert_same(m[1].data.cpu().numpy(), exp, "forward")
    Transposition(m[0], m[1], wire_dtype="float32").execute()
    assert_same(m[0].data.cpu().numpy(), ref_round(src, "f64_f32"), "back")


def test_execute_without_set_buffers_sizes_fallback_in_wire_bytes(
        oracle_lib_path):
    """An aliased world-1 plan stages its self block; with no
    pa_plan_set_buffers the engine allocates that staging itself, in wire
    bytes."""
    wname, srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), oracle_lib_path)
    s, d = srcs[0], dsts[0]
    p = native.NativePlan(s.pencil, d.pencil, 0, 8, aliased=True,
                          wire=native.WIRE_F64_F32)
    sb, rb = p.buffer_sizes()
    assert (sb, rb) == (0, 4 * len(s))
    p.execute(s.data.data_ptr(), d.data.data_ptr(), 0)
    p.wait(0)
    _check_e2e(dsts, raws, exp)
