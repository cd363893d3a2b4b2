"""Scaled transposes (dest = alpha * T(src)) on one MI355X: the scaling
kernels through pa_device_copy_scale, through the stage API as a multi-rank
run, through Transposition / MultiTransposition end to end, on a live plan
whose alpha changes, and past the gridDim.x split and byte 2^32.

Every case asserts its selection or launch rows through the queries with the
real pointers before launching, prefills destinations and staging with 0xAB
behind 256-byte guards, and compares whole buffers as bit patterns (NaN for
NaN-ness) with references that are not the code under test: numpy on the real
view and the C oracle on the scaled input."""

import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import (  # noqa: E402
    DEV, assert_split, batch_transpose_desc, extent as elem_extent,
    far_window, host_ref, max_x, run_far,
)
from pencilarrays_amd import (  # noqa: E402
    ManyPencilArray, MultiTransposition, Pencil, PencilArray, Topology,
    Transposition, fourier_keep, native,
)
from scale_gpu_util import (  # noqa: E402
    CODE, expected_of, ref_copy_scale, run_copy_scale, run_stage_sim_scaled,
)
from scale_util import (  # noqa: E402
    ALPHAS, F32, F64, GEN, KINDS, LIN, TILE, assert_same, expected_rows,
    expected_scaled, kind_parents, pencils, plan_of, plan_rows, ref_scale,
    seeded_patterns, seeded_values, specials, tile_shape,
)
from wire_gpu_util import GUARD, SENT, sentinel, transpose_desc  # noqa: E402

ID3 = (0, 1, 2)
PACK, LOCAL, UNPACK = (native.STAGE_PACK, native.STAGE_LOCAL,
                       native.STAGE_UNPACK)
REALS = [np.float32, np.float64]
SID = lambda s: np.dtype(s).name  # noqa: E731
THIRD = 1.0 / 3.0


def _rows(l):
    return [(x.kind, x.grouped, x.entries) for x in l]


# ---- 1. special values, 1-D -----------------------------------------------------

@pytest.mark.parametrize("alpha", ALPHAS, ids=repr)
@pytest.mark.parametrize("S", REALS, ids=SID)
def test_special_values_1d(S, alpha):
    src = np.concatenate([specials(S), seeded_patterns(4096, S, 0xA1FA),
                          specials(S)])
    vmax = 16 // np.dtype(S).itemsize
    n = len(src) // vmax * vmax
    run_copy_scale(((n,), (1,), 0, (1,), 0), S, 1, alpha, 0, LIN, vmax,
                   slack=0, src=src[:n])


# ---- 2. linear windows at each V ------------------------------------------------

def _lin(n0=64, n1=5, sp=72, dp=80, soff=0, doff=0):
    return ((n0, n1), (1, sp), soff, (1, dp), doff)


@pytest.mark.parametrize("S", REALS, ids=SID)
def test_linear_windows_each_v(S):
    vmax = 16 // np.dtype(S).itemsize
    run_copy_scale(_lin(), S, 1, THIRD, 10, LIN, vmax)
    v = vmax
    while v > 1:
        h = v // 2  # each misalignment alone lowers V to h
        run_copy_scale(_lin(), S, 1, THIRD, 11, LIN, h, src_lead=h)
        run_copy_scale(_lin(), S, 1, THIRD, 12, LIN, h, dst_lead=h)
        run_copy_scale(_lin(soff=h), S, 1, THIRD, 13, LIN, h)
        run_copy_scale(_lin(doff=h), S, 1, THIRD, 14, LIN, h)
        run_copy_scale(_lin(sp=72 + h), S, 1, THIRD, 15, LIN, h)
        run_copy_scale(_lin(dp=80 + h), S, 1, THIRD, 16, LIN, h)
        run_copy_scale(_lin(n0=64 - h), S, 1, THIRD, 17, LIN, h)
        v = h
    # elements of several scalars join the run; more than one workgroup
    run_copy_scale(_lin(n0=300, n1=7, sp=300, dp=301), S, 2, -2.0, 18, LIN, 2)
    run_copy_scale(_lin(n0=301, n1=7, sp=301, dp=303), S, 3, -2.0, 19, LIN, 1)


# ---- 3. the tile ------------------------------------------------------------------

def _tile_case(S, nscal, n0, nta, nb, seed, window=False, ta_pos=1,
               src_lead=0, dst_lead=0):
    sp = n0 + (3 if window else 0)
    dp = nta + (5 if window else 0)
    desc = transpose_desc(n0, nta, nb, sp, 2 if window else 0, dp,
                          1 if window else 0, ta_pos)
    want = TILE if n0 > 1 and nta > 1 else None  # a unit extent drops out
    return run_copy_scale(desc, S, nscal, THIRD, seed, want,
                          src_lead=src_lead, dst_lead=dst_lead)


@pytest.mark.parametrize("nscal", [1, 2, 3, 4])
@pytest.mark.parametrize("S", REALS, ids=SID)
def test_tile_extent_sweep(S, nscal):
    code = CODE[np.dtype(S)]
    q = native.copy_kernel_kind_scale(transpose_desc(9, 9, 1, 9, 0, 9, 0),
                                      code, nscal)
    assert q.kind == TILE and (q.tile_i, q.tile_j) == tile_shape(code, nscal)
    Ti, Tj = q.tile_i, q.tile_j
    e0 = [1, Ti - 1, Ti, Ti + 1, 2 * Ti + 1]
    e1 = [1, Tj - 1, Tj, Tj + 1, 2 * Tj + 1]
    if nscal == 1:  # every pair
        pairs = [(a, b) for a in e0 for b in e1]
    else:           # every extent of one axis against T + 1 of the other
        pairs = [(a, Tj + 1) for a in e0] + [(Ti + 1, b) for b in e1]
    for i, (n0, nta) in enumerate(pairs):
        _tile_case(S, nscal, n0, nta, 1, 100 + i)
    # windows, ta behind the batch axis, batch 3, base pointers one scalar in
    _tile_case(S, nscal, Ti + 1, Tj + 1, 3, 200, window=True)
    _tile_case(S, nscal, Ti + 1, Tj - 1, 3, 201, ta_pos=2)
    _tile_case(S, nscal, 2 * Ti + 1, Tj + 1, 3, 202, window=True, ta_pos=2)
    _tile_case(S, nscal, Ti - 1, 2 * Tj + 1, 3, 203, src_lead=1, dst_lead=1)
    _tile_case(S, nscal, Ti + 1, Tj + 1, 2, 204, window=True, src_lead=1)


@pytest.mark.parametrize("S", REALS, ids=SID)
def test_generic(S):
    # more than four scalars per element; no contiguous source axis
    run_copy_scale(transpose_desc(37, 41, 3, 37, 0, 41, 0), S, 6, THIRD, 300,
                   GEN)
    run_copy_scale(((37, 41), (2, 80), 1, (41, 1), 0), S, 1, -2.0, 301, GEN)
    run_copy_scale(((37, 41), (2, 80), 1, (43, 1), 2), S, 2, 0.5, 302, GEN)


# ---- 4. the stage API as a multi-rank run on one GPU ------------------------------

STAGE_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    # empty ranks: 3 planes over 4 ranks
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ()),
]
ALPHA_N = 1.0 / (130 * 67 * 35)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["f64", "c128", "f32", "3xf32"])
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_stage_api_multirank_on_one_gpu(cfg, kind, n, oracle_lib_path):
    run_stage_sim_scaled(cfg, kind, n, ALPHA_N, oracle_lib_path)


def test_stage_api_aliased(oracle_lib_path):
    """PA_PLAN_ALIASED: the self pack stays the ordinary kernel, the self
    unpack scales."""
    seen = []

    def hook(r, rows):
        seen.append(bool(rows[LOCAL]))
        assert all(l.kind in (LIN, TILE, GEN) for l in rows[LOCAL])

    run_stage_sim_scaled(STAGE_CFGS[0], "f64", 3, THIRD, oracle_lib_path,
                         aliased=True, rows_hook=hook)
    assert any(seen)


def test_stage_api_keep_fill_zero(oracle_lib_path):
    cfg = STAGE_CFGS[0]
    keep = fourier_keep(cfg[0], [5, 6, None], real_dim=0)
    fills = []

    def hook(r, rows):
        fills.append([l for l in rows[LOCAL]
                      if l.kind == native.KERNEL_FILL])

    run_stage_sim_scaled(cfg, "c128", 2, THIRD, oracle_lib_path, keep=keep,
                         rows_hook=hook)
    assert any(fills) and all(len(f) <= 1 and all(l.grouped for l in f)
                              for f in fills)


# ---- 5. grouped rows -----------------------------------------------------------------

def _slab(n0, n1, n2, P):
    return ((n0, n1, n2), (P,), (1,), ID3, (0,), (1, 0, 2), ())


@pytest.mark.parametrize("kind", ["f64", "f32", "c64"])
@pytest.mark.parametrize("P", [2, 3])
def test_ragged_tiles_inside_one_group(P, kind, oracle_lib_path):
    """An unpack entry is (my dim-0 range) x (the peer's dim-1 range).  Every
    entry has two or more tiles along both axes and a ragged last tile along
    axis 0.  P = 2: dim-1 ranges 67 and 68.  P = 3: ranges 128, 128, 129, so
    entries of different block counts (2 and 3 tiles along ta) sit in one
    grouped row; the third ends in a one-wide tile."""
    code, nscal = KINDS[kind][3], KINDS[kind][4]
    ti, tj = tile_shape(code, nscal)
    assert tj == 64
    n0 = P * (ti + 3) + 1
    n1 = 135 if P == 2 else 385
    cfg = _slab(n0, n1, 2, P)
    n = 2
    seen = set()

    def hook(r, rows):
        assert _rows(rows[UNPACK]) == [(TILE, True, n * (P - 1))], rows
        assert _rows(rows[LOCAL]) == [(TILE, True, n)], rows
        seen.add(rows[UNPACK][0].workgroups)

    run_stage_sim_scaled(cfg, kind, n, THIRD, oracle_lib_path, rows_hook=hook)
    if P == 3:  # ranks see peers of 2+3, 2+3 and 2+2 tiles along ta
        assert len(seen) > 1, seen


def test_two_linear_rows_of_different_v_in_one_stage(oracle_lib_path):
    """Same decomposition, no permutation: the local copy of every field is
    one run.  Field 1 of 3 starts one f64 into its allocations and scales one
    scalar per access, the others two."""
    cfg = ((16, 22, 41), (2, 2), (1, 2), ID3, (1, 2), ID3, ())

    def hook(r, rows):
        assert _rows(rows[LOCAL]) == [(LIN, True, 2), (LIN, True, 1)], rows
        assert rows[PACK] == [] and rows[UNPACK] == []

    run_stage_sim_scaled(cfg, "f64", 3, THIRD, oracle_lib_path, lead={1: 1},
                         rows_hook=hook)


# ---- 6. end to end, world 1 -----------------------------------------------------------

E2E_DIMS = (130, 67, 35)


def _e2e(kind, po, alpha, oracle_lib_path, n=1, lead=None, keep=None):
    """Sources, 0xAB-prefilled destinations and the expectation of a world-1
    scaled transpose of ``n`` fields; ``lead[f]``: field ``f`` starts that
    many bytes into its allocations."""
    dtype, elem = KINDS[kind][:2]
    lead = lead or {}
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2), po, ())
    Pi, Po = pencils(cfg)
    parents = kind_parents(kind, cfg, n, oracle_lib_path)
    exp = expected_of(kind, parents, cfg, alpha, keep, oracle_lib_path)
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
    return srcs, dsts, raws, exp


def _check_e2e(dsts, raws, exp):
    torch.cuda.synchronize()
    for f, (d, (raw, lb, nb)) in enumerate(zip(dsts, raws)):
        assert_same(d.data.cpu().numpy(), exp[f][0], f"field {f}")
        assert raw.numel() == lb + nb + GUARD
        assert (raw[:lb] == SENT).all().item(), f"field {f} lead"
        assert (raw[lb + nb:] == SENT).all().item(), f"field {f} guard"


def _local_rows(t, kind, srcs, dsts, alpha, keep=None):
    """The rows of a (Multi)Transposition's native plan, whose native side is
    made here as its first execute would, against the partition built from
    the plan without a scale."""
    multi = isinstance(t, MultiTransposition)
    if t._native is None:
        t._native = (native.NativeMultiTransposition if multi
                     else native.NativeTransposition)(t)
    nat = t._native.native
    code, nscal = KINDS[kind][3], KINDS[kind][4]
    assert nat.plan_scale() == (code, alpha)
    sp = [s.data.data_ptr() for s in srcs]
    dp = [d.data.data_ptr() for d in dsts]
    s0 = srcs[0]
    plain = native.NativePlan(s0.pencil, dsts[0].pencil, 0,
                              s0.data.element_size(), aliased=t.plan.aliased,
                              ncomp=s0.ncomp, keep=keep)
    n = len(srcs)
    rows = plan_rows(nat, n, sp, dp)
    assert rows == expected_rows(plain, n, code, nscal, sp, dp), rows
    assert rows[PACK] == [] and rows[UNPACK] == []
    return rows[LOCAL]


@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
@pytest.mark.parametrize("kind", ["f32", "c64", "f64", "c128"])
def test_world1_transposition(kind, po, oracle_lib_path):
    srcs, dsts, raws, exp = _e2e(kind, po, ALPHA_N, oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], scale=ALPHA_N)
    rows = _local_rows(t, kind, srcs, dsts, ALPHA_N)
    assert _rows(rows) == [(LIN if po == ID3 else TILE, True, 1)]
    t.execute()
    _check_e2e(dsts, raws, exp)
    # a repeated call reuses the stage table
    nat = t._native.native
    builds = nat.stage_table_builds()
    assert builds >= 1
    t.execute()
    assert nat.stage_table_builds() == builds
    _check_e2e(dsts, raws, exp)


def test_world1_async_then_wait(oracle_lib_path):
    srcs, dsts, raws, exp = _e2e("f64", (1, 2, 0), THIRD, oracle_lib_path)
    t = Transposition(dsts[0], srcs[0], scale=THIRD)
    _local_rows(t, "f64", srcs, dsts, THIRD)
    t.execute(sync=False)
    t.wait()
    _check_e2e(dsts, raws, exp)


def test_world1_inplace_there_and_back():
    """x -> y -> x in place over a ManyPencilArray pair: the reference
    multiply applied twice."""
    topo = Topology((1, 1))
    Pi = Pencil(topo, E2E_DIMS, (1, 2))
    Po = Pencil(topo, E2E_DIMS, (0, 2), permute=(1, 2, 0))
    m = ManyPencilArray((Pi, Po), 0, dtype=torch.float64, device="cuda:0")
    orig = seeded_values(Pi.length_local(0), np.float64, 77)
    m.first.data.copy_(torch.from_numpy(orig))
    for i, j in ((0, 1), (1, 0)):
        t = Transposition(m[j], m[i], scale=THIRD)
        assert t.plan.aliased
        t._native = native.NativeTransposition(t)
        nat = t._native.native
        assert nat.plan_scale() == (F64, THIRD)
        sp, dp = [m[i].data.data_ptr()], [m[j].data.data_ptr()]
        assert all(l.kind not in (LIN, TILE, GEN)
                   for l in nat.stage_launches(1, PACK, sp, dp))
        assert _rows(nat.stage_launches(1, LOCAL, sp, dp)) in \
            ([(TILE, True, 1)], [(LIN, True, 1)])
        t.execute()
    torch.cuda.synchronize()
    assert_same(m.first.data.cpu().numpy(),
                ref_scale(ref_scale(orig, THIRD), THIRD))


@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
def test_world1_multitransposition_one_field_8_bytes_off(po, oracle_lib_path):
    srcs, dsts, raws, exp = _e2e("f64", po, THIRD, oracle_lib_path, n=3,
                                 lead={1: 8})
    mt = MultiTransposition(dsts, srcs, scale=THIRD)
    rows = _local_rows(mt, "f64", srcs, dsts, THIRD)
    if po == ID3:  # the field 8 bytes off scales one scalar per access
        assert _rows(rows) == [(LIN, True, 2), (LIN, True, 1)]
    else:
        assert _rows(rows) == [(TILE, True, 3)]
    mt.execute()
    _check_e2e(dsts, raws, exp)


def test_world1_keep_with_scale(oracle_lib_path):
    keep = fourier_keep(E2E_DIMS, [40, 20, 11], real_dim=0)
    srcs, dsts, raws, exp = _e2e("c128", (1, 2, 0), ALPHA_N, oracle_lib_path,
                                 keep=keep)
    t = Transposition(dsts[0], srcs[0], keep=keep, scale=ALPHA_N)
    rows = _local_rows(t, "c128", srcs, dsts, ALPHA_N, keep=keep)
    assert rows[-1].kind == native.KERNEL_FILL and rows[-1].grouped
    assert rows[:-1] and all(l.kind in (LIN, TILE) and l.grouped
                             for l in rows[:-1])
    t.execute()
    _check_e2e(dsts, raws, exp)


# ---- 7. alpha changes on a live plan ---------------------------------------------------

def test_changing_alpha_on_a_live_plan(oracle_lib_path):
    kind, po = "f64", (1, 2, 0)
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2), po, ())
    parents = kind_parents(kind, cfg, 1, oracle_lib_path)
    src = torch.from_numpy(parents[0][0].copy().view(np.uint8)).to("cuda:0")
    nb = parents[0][0].nbytes
    stream = torch.cuda.current_stream().cuda_stream
    p = plan_of(cfg, 0, kind, alpha=0.5)
    plain = plan_of(cfg, 0, kind)

    for_dst = {}

    def fixed(plan):
        # one destination per plan, so the stage table's key stays the same
        raw = for_dst.setdefault(id(plan), sentinel(nb))
        raw.fill_(SENT)
        sp, dp = [src.data_ptr()], [raw.data_ptr()]
        plan.execute_many(sp, dp, stream)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        assert (got[nb:] == SENT).all()
        return got[:nb].view(np.float64)

    exp = lambda a: expected_scaled(kind, parents, cfg, a,  # noqa: E731
                                    oracle_lib_path)[0][0]
    assert _rows(p.stage_launches(1, LOCAL, [src.data_ptr()], None)) == \
        [(TILE, True, 1)]
    assert_same(fixed(p), exp(0.5), "alpha 0.5")
    builds = p.stage_table_builds()
    assert builds >= 1 and p.stage_table_count() >= 1
    p.set_scale(F64, 0.25)
    assert p.stage_table_count() >= 1
    assert_same(fixed(p), exp(0.25), "alpha 0.25")
    assert p.stage_table_builds() == builds
    p.set_scale(F64, 1.0)
    assert p.stage_table_count() == 0 and p.plan_scale() is None
    rows = p.stage_launches(1, LOCAL, [src.data_ptr()], None)
    assert rows == plain.stage_launches(1, LOCAL, [src.data_ptr()], None)
    got = fixed(p)
    assert p.stage_table_builds() > builds
    want = fixed(plain)
    assert got.tobytes() == want.tobytes()
    assert_same(got, exp(1.0), "alpha 1.0")


# ---- 8. launch geometry ------------------------------------------------------------------

MX1024 = max_x(1024)


@pytest.mark.parametrize("S", REALS, ids=SID)
def test_tile_past_the_split(S):
    """k_scale_tile, one workgroup per 2 x 2 batch, more workgroups than
    gridDim.x holds."""
    S = np.dtype(S)
    desc = batch_transpose_desc(2, MX1024 + 5)
    dims, sstr, soff, dstr, doff = desc
    B = S.itemsize
    src = seeded_values(elem_extent(dims, sstr, soff), S, 2600)
    dst_n = elem_extent(dims, dstr, doff) + 4
    exp = np.full(dst_n * B, SENT, dtype=np.uint8)
    host_ref(desc, ref_scale(src, THIRD).view(np.uint8), exp, B)
    s_t = torch.from_numpy(src.view(np.uint8)).to(DEV)
    d_t = torch.full((exp.nbytes + GUARD,), SENT, dtype=torch.uint8,
                     device=DEV)
    try:
        k = native.copy_kernel_kind_scale(desc, CODE[S], 1, s_t.data_ptr(),
                                          d_t.data_ptr())
        assert k.kind == TILE, k
        wg = math.ceil(2 / k.tile_i) * math.ceil(2 / k.tile_j) * dims[2]
        assert wg == 4194308
        assert_split(wg, 1024)
        native.device_copy_scale(desc, CODE[S], 1, THIRD, s_t.data_ptr(),
                                 d_t.data_ptr())
        torch.cuda.synchronize()
        got = d_t.cpu().numpy()
        assert (got[exp.nbytes:] == SENT).all()
        assert_same(got[:exp.nbytes].view(S), exp.view(S))
    finally:
        s_t = d_t = None
        torch.cuda.empty_cache()


def test_grouped_tile_row_straddles_the_grid_row(oracle_lib_path):
    """Three f64 fields, x-pencil to y-pencil with permute (1, 0, 2): one
    grouped SCALE_TILE row of three entries whose workgroups pass the
    gridDim.x limit, the grid-row boundary strictly inside the third."""
    dims, wg, n, kind = (2, 2, 1398103), 4194309, 3, "f64"
    cfg = (dims, (1, 1), (1, 2), ID3, (0, 2), (1, 0, 2), ())
    parents = kind_parents(kind, cfg, n, oracle_lib_path)
    exp = expected_scaled(kind, parents, cfg, THIRD, oracle_lib_path)
    plan = plan_of(cfg, 0, kind, alpha=THIRD)
    srcs = [torch.from_numpy(parents[f][0].view(np.uint8)).to(DEV)
            for f in range(n)]
    dsts = [sentinel(exp[f][0].nbytes) for f in range(n)]
    sp = [t.data_ptr() for t in srcs]
    dp = [t.data_ptr() for t in dsts]
    try:
        rows = plan.stage_launches(n, LOCAL, sp, dp)
        assert [(l.kind, l.grouped, l.entries, l.workgroups)
                for l in rows] == [(TILE, True, 3, wg)], rows
        assert_split(wg, 1024)
        per = wg // 3
        assert 3 * per == wg and 2 * per < MX1024 < wg - 1
        assert rows == expected_rows(plan_of(cfg, 0, kind), n, F64, 1, sp,
                                     dp)[LOCAL]
        plan.execute_many(sp, dp, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for f in range(n):
            got = dsts[f].cpu().numpy()
            nb = exp[f][0].nbytes
            assert (got[nb:] == SENT).all(), f
            assert_same(got[:nb].view(np.float64), exp[f][0], f"field {f}")
    finally:
        del srcs, dsts, plan
        torch.cuda.empty_cache()


HUGE_BYTES = (1 << 33) + (1 << 21)


@pytest.fixture(scope="module")
def huge():
    """One 8 GiB (and a little) allocation that every far-offset case takes
    a prefix of as its huge side."""
    t = torch.empty(HUGE_BYTES, dtype=torch.uint8, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


# family: (kind, shape, source pitch, destination pitch)
FAR_SCALE = {"linear": (LIN, "l", 76, 72), "tile": (TILE, "t", 72, 68)}


@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("family", list(FAR_SCALE))
@pytest.mark.parametrize("S", REALS, ids=SID)
def test_window_past_2e32_bytes(S, family, side, huge):
    """A (70, 66, 3) window whose offset lies past byte 2^32 of the huge
    side, one side at a time."""
    S = np.dtype(S)
    kind, shape, sp, dp = FAR_SCALE[family]
    B = S.itemsize
    win = far_window(shape, sp, dp, False, side, "offset", (1 << 32) // B)
    seed = [3700]

    def make_src(count):
        seed[0] += 1
        return seeded_values(count, S, seed[0]).view(np.uint8)

    def ref(d2, s, d):
        ref_copy_scale(d2, s.view(S), d.view(S), 1, THIRD)

    def select(desc, s, d):
        k = native.copy_kernel_kind_scale(desc, CODE[S], 1, s, d)
        assert k.kind == kind, (desc, k)

    def same(got, exp, what):
        assert_same(got.view(S), exp.view(S), what)

    run_far(win, B, B, huge, make_src, ref, select,
            lambda desc, s, d: native.device_copy_scale(desc, CODE[S], 1,
                                                        THIRD, s, d),
            same, 1 << 32)
