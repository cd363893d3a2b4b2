"""Scaled split and join transposes, host side (no GPU).

The multiply is checked against numpy on the real view, the placement
against the C oracle per component on the reference-scaled copies, the
staging against run_transpose_sim_many: a join's buffers are the unscaled
join's, a split's are those of the n-field plan on the scaled copies.  Then
the native *_scaled calls' refusals, host only."""

from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from scale_util import ALPHAS, seeded_patterns, specials
from soa_scale_util import (
    KINDS, pick_alpha, same, scale_bytes, scaled_join_case, scaled_split_case,
)
from soa_util import component, interleave, join_case, split_case
from many_util import expected_dests
from test_soa_cpu import CONFIGS, _ids
from pencilarrays_amd import (
    JoinTransposition,
    Pencil,
    PencilArray,
    SplitTransposition,
    Topology,
    native,
    run_transpose_sim_join,
    run_transpose_sim_many,
    run_transpose_sim_split,
    transpose_join_into,
    transpose_split_into,
)

ID3 = (0, 1, 2)
KIND_IDS = sorted(KINDS)


def _pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po), topo.nranks, extra)


def _arr(P, r, raw, kind, extra, elem_dims=()):
    return PencilArray(P, r, raw.view(KINDS[kind][0]).copy(), extra,
                       elem_dims)


def _zeros(P, r, nbytes, kind, extra, elem_dims=()):
    dt = KINDS[kind][0]
    return PencilArray(P, r, np.zeros(nbytes // dt.itemsize, dtype=dt), extra,
                       elem_dims)


def _many_staging(cfg, kind, srcs_c, exp_c):
    """Staging of the ordinary UNSCALED n-field plan on scalar sources
    ``srcs_c[c][r]`` (bytes), after checking its destinations."""
    Pi, Po, nr, extra = _pencils(cfg)
    n = len(srcs_c)
    srcs = [[_arr(Pi, r, srcs_c[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp_c[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_many(dsts, srcs, staging_out=staging)
    for r in range(nr):
        for c in range(n):
            assert dsts[r][c].data.tobytes() == exp_c[c][r].tobytes()
    return staging


def _same_staging(a, b, kind):
    for side in ("send", "recv"):
        assert len(a[side]) == len(b[side])
        for r, (x, y) in enumerate(zip(a[side], b[side])):
            same(x, y, kind, f"{side} buffer of rank {r}")


def _bytes_staging(a, b):
    for side in ("send", "recv"):
        assert len(a[side]) == len(b[side])
        for x, y in zip(a[side], b[side]):
            assert x.tobytes() == y.tobytes(), side


# ---- 1. the multiply, through the numpy classes in world 1 ----------------

W1_DIMS = (50, 25, 41)     # 51250 elements of 2 components


def _w1_cfg(permuted=True):
    return (W1_DIMS, (1, 1), (1, 2), ID3, (0, 2),
            (1, 2, 0) if permuted else ID3, ())


@pytest.mark.parametrize("kind", KIND_IDS)
def test_specials_and_patterns_through_the_classes(kind, oracle_lib_path):
    """The specials and 10^5 seeded bit patterns per real type, times the six
    alphas, through JoinTransposition and SplitTransposition on numpy arrays;
    a complex scalar is two real ones."""
    dt, ssz, R, _ = KINDS[kind]
    n = 2
    cfg = _w1_cfg()
    Pi, Po, _, extra = _pencils(cfg)
    nreal = math.prod(W1_DIMS) * n * (ssz // R.itemsize)
    sp = specials(R)
    assert nreal >= 100000 + len(sp)
    vals = seeded_patterns(nreal, R, 0x5CA1E)
    vals[:len(sp)] = sp
    raw = vals.view(np.uint8)
    comps = [[component(raw, ssz, n, c)] for c in range(n)]
    for alpha in ALPHAS:
        scaled = [[scale_bytes(x[0], kind, alpha)] for x in comps]
        # split: the array of structs is `raw`, on the input pencil
        exp = expected_dests(scaled, cfg, ssz, oracle_lib_path)
        src = _arr(Pi, 0, raw, kind, extra, (n,))
        dsts = [_zeros(Po, 0, len(exp[c][0]), kind, extra) for c in range(n)]
        SplitTransposition(dsts, src, scale=alpha).execute()
        for c in range(n):
            same(dsts[c].data, exp[c][0], kind, f"split {alpha} field {c}")
        assert src.data.tobytes() == raw.tobytes()
        # join: the same components as scalar fields on the input pencil
        srcs = [_arr(Pi, 0, comps[c][0], kind, extra) for c in range(n)]
        dst = _zeros(Po, 0, len(raw), kind, extra, (n,))
        JoinTransposition(dst, srcs, scale=alpha).execute()
        same(dst.data, interleave([exp[c][0] for c in range(n)], ssz), kind,
             f"join {alpha}")


# ---- 2. the simulations: result, and what staging holds -------------------

CASES = [(ci, kind, n) for ci in range(len(CONFIGS)) for kind in KIND_IDS
         for n in (2, 3, 4)]


def _case_id(v):
    ci, kind, n = v
    return f"{_ids(CONFIGS[ci])}-{kind}-n{n}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_split_sim_scaled(case, oracle_lib_path):
    ci, kind, n = case
    cfg = CONFIGS[ci]
    alpha = pick_alpha(ci + n + KIND_IDS.index(kind))
    Pi, Po, nr, extra = _pencils(cfg)
    aos, scaled, exp = scaled_split_case(cfg, kind, n, alpha,
                                         oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging, scale=alpha)
    for r in range(nr):
        for c in range(n):
            same(dsts[r][c].data, exp[c][r], kind, (r, c))
        assert srcs[r].data.tobytes() == aos[r].tobytes()  # source untouched
    # the buffers: those of the n-field plan on the SCALED component copies
    _same_staging(staging, _many_staging(cfg, kind, scaled, exp), kind)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_join_sim_scaled(case, oracle_lib_path):
    ci, kind, n = case
    cfg = CONFIGS[ci]
    alpha = pick_alpha(ci + n + KIND_IDS.index(kind) + 3)
    Pi, Po, nr, extra = _pencils(cfg)
    fields, scaled, exp_c, exp = scaled_join_case(cfg, kind, n, alpha,
                                                  oracle_lib_path)

    def run(scale):
        srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
                for r in range(nr)]
        dsts = [_zeros(Po, r, len(exp[r]), kind, extra, (n,))
                for r in range(nr)]
        staging = {}
        run_transpose_sim_join(dsts, srcs, staging_out=staging, scale=scale)
        return dsts, staging

    dsts, staging = run(alpha)
    for r in range(nr):
        same(dsts[r].data, exp[r], kind, r)
    # every buffer byte-identical to the unscaled join's
    _bytes_staging(staging, run(None)[1])


# ---- 3, 4. a scaled side facing an ordinary n-field stage ------------------

@pytest.mark.parametrize("kind", ["f64", "c64"])
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
def test_ordinary_unpack_faces_a_scaled_split_pack(cfg, kind,
                                                   oracle_lib_path):
    """The scaled split runs its pack, the exchange and its local copy; the
    unpack is the ordinary n-field one, by run_transpose_sim_many's own
    descriptors, and delivers the scaled fields."""
    from pencilarrays_amd.copyexec import apply_copy
    from pencilarrays_amd.plan import build_plan, stage_descs
    n, alpha = 3, 1.0 / 3.0
    Pi, Po, nr, extra = _pencils(cfg)
    aos, _, exp = scaled_split_case(cfg, kind, n, alpha, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging, scale=alpha,
                            stages=("pack", "exchange", "local"))
    for r in range(nr):
        plan = build_plan(Pi, Po, r, extra)
        for c in range(n):
            for _, d in stage_descs(plan, n, c, 2):
                apply_copy(d, staging["recv"][r], dsts[r][c].data)
            same(dsts[r][c].data, exp[c][r], kind, (r, c))


@pytest.mark.parametrize("kind", ["f64", "c64"])
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
def test_scaled_join_unpack_faces_an_ordinary_pack(cfg, kind,
                                                   oracle_lib_path):
    """The ordinary n-field pack and exchange fill the buffers (unscaled);
    the scaled join runs only its local copy and its unpack on them."""
    n, alpha = 3, -2.0
    ssz = KINDS[kind][1]
    Pi, Po, nr, extra = _pencils(cfg)
    fields, _, _, exp = scaled_join_case(cfg, kind, n, alpha,
                                         oracle_lib_path)
    plain_c = expected_dests(fields, cfg, ssz, oracle_lib_path)
    staging = _many_staging(cfg, kind, fields, plain_c)
    srcs = [[_arr(Pi, r, fields[c][r], kind, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_zeros(Po, r, len(exp[r]), kind, extra, (n,)) for r in range(nr)]
    run_transpose_sim_join(dsts, srcs, stages=("local", "unpack"),
                           staging_in=staging, scale=alpha)
    for r in range(nr):
        same(dsts[r].data, exp[r], kind, r)


# ---- 5. split by 0.5, join by 2.0 -----------------------------------------

@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5], CONFIGS[9]],
                         ids=_ids)
def test_split_half_then_join_twice_is_the_identity(cfg, kind,
                                                    oracle_lib_path):
    """Values in [1, 2): halving and doubling are both exact."""
    n = 3
    dt, ssz, R, _ = KINDS[kind]
    Pi, Po, nr, extra = _pencils(cfg)
    aos, _, exp = split_case(cfg, ssz, n, oracle_lib_path)
    rng = np.random.default_rng(0xD0)
    aos = [(1.0 + rng.random(len(a) // R.itemsize)).astype(R).view(np.uint8)
           for a in aos]
    assert all(((a.view(R) >= 1) & (a.view(R) < 2)).all() for a in aos)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    mids = [[_zeros(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    run_transpose_sim_split(mids, srcs, scale=0.5)
    back = [_zeros(Pi, r, len(aos[r]), kind, extra, (n,)) for r in range(nr)]
    run_transpose_sim_join(back, mids, scale=2.0)
    for r in range(nr):
        assert back[r].data.tobytes() == aos[r].tobytes(), r
        if len(aos[r]):   # and the middle really was halved
            assert (mids[r][0].data.view(R) < 1).all()


# ---- 6. scale=1.0 and None are the unscaled run ---------------------------

@pytest.mark.parametrize("scale", [None, 1.0, 1], ids=str)
@pytest.mark.parametrize("kind", ["f32", "c128"])
def test_scale_one_and_none_are_the_unscaled_run(kind, scale,
                                                 oracle_lib_path):
    """Random bit patterns hold NaNs with payloads: every byte comes through,
    in the simulations (staging included) and in the classes."""
    n, cfg = 3, CONFIGS[0]
    ssz = KINDS[kind][1]
    Pi, Po, nr, extra = _pencils(cfg)
    aos, comps, exp = split_case(cfg, ssz, n, oracle_lib_path)
    R = KINDS[kind][2]
    assert any(np.isnan(a.view(R)).any() for a in aos)
    srcs = [_arr(Pi, r, aos[r], kind, extra, (n,)) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
            for r in range(nr)]
    st, st0 = {}, {}
    run_transpose_sim_split(dsts, srcs, staging_out=st, scale=scale)
    for r in range(nr):
        for c in range(n):
            assert dsts[r][c].data.tobytes() == exp[c][r].tobytes(), (r, c)
    run_transpose_sim_split(
        [[_zeros(Po, r, len(exp[c][r]), kind, extra) for c in range(n)]
         for r in range(nr)], srcs, staging_out=st0)
    _bytes_staging(st, st0)
    back = [_zeros(Pi, r, len(aos[r]), kind, extra, (n,)) for r in range(nr)]
    run_transpose_sim_join(back, dsts, scale=scale)
    for r in range(nr):
        assert back[r].data.tobytes() == aos[r].tobytes(), r
    # the classes, world 1
    cfg1 = ((13, 11, 7), (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    Pi, Po, _, extra = _pencils(cfg1)
    aos, _, exp = split_case(cfg1, ssz, n, oracle_lib_path)
    src = _arr(Pi, 0, aos[0], kind, extra, (n,))
    out = [_zeros(Po, 0, len(exp[c][0]), kind, extra) for c in range(n)]
    t = SplitTransposition(out, src, scale=scale)
    assert t.scale is None
    t.execute()
    for c in range(n):
        assert out[c].data.tobytes() == exp[c][0].tobytes()
    b = _zeros(Pi, 0, len(aos[0]), kind, extra, (n,))
    j = JoinTransposition(b, out, scale=scale)
    assert j.scale is None
    j.execute()
    assert b.data.tobytes() == aos[0].tobytes()


def test_classes_keep_the_scale_and_wait():
    cfg = ((13, 11, 7), (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    Pi, Po, _, _ = _pencils(cfg)
    a = PencilArray.empty(Pi, 0, np.complex64, elem_dims=(2,))
    fs = [PencilArray.empty(Po, 0, np.complex64) for _ in range(2)]
    a.data[...] = 3 + 4j
    t = SplitTransposition(fs, a, scale=0.5)
    assert t.scale.alpha == 0.5 and t.scale.code == native.SCALAR_F32
    assert t.execute(sync=False) is t.dests and t.wait() is t
    assert (fs[0].data == 1.5 + 2j).all() and (fs[1].data == 1.5 + 2j).all()
    j = JoinTransposition(a, fs, scale=-2.0)
    assert j.scale.alpha == -2.0 and j.execute() is a
    assert (a.data == -3 - 4j).all()


# ---- 7. gloo, world 2 -----------------------------------------------------

def _gloo_worker(rank, world, port, lib):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        kind, n = "f64", 3
        cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        Pi, Po, _, extra = _pencils(cfg)
        aos, _, exp = scaled_split_case(cfg, kind, n, 1.0 / 3.0, lib)
        src = _arr(Pi, rank, aos[rank], kind, extra, (n,))
        dsts = [_zeros(Po, rank, len(exp[c][rank]), kind, extra)
                for c in range(n)]
        transpose_split_into(dsts, src, scale=1.0 / 3.0)
        for c in range(n):
            same(dsts[c].data, exp[c][rank], kind, (rank, c))
        fields, _, _, expj = scaled_join_case(cfg, kind, n, -2.0, lib)
        srcs = [_arr(Pi, rank, fields[c][rank], kind, extra)
                for c in range(n)]
        dst = _zeros(Po, rank, len(expj[rank]), kind, extra, (n,))
        transpose_join_into(dst, srcs, scale=-2.0)
        same(dst.data, expj[rank], kind, rank)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2(oracle_lib_path):
    mp.spawn(_gloo_worker, args=(2, 31500 + os.getpid() % 2000,
                                 oracle_lib_path), nprocs=2, join=True)


# ---- 8. native, host only --------------------------------------------------

F32, F64 = native.SCALAR_F32, native.SCALAR_F64
FAKE = 4096   # aligned addresses that are never touched


def _slab(**kw):
    topo = Topology((2,))
    dims = (8, 6, 4)
    return native.NativePlan(Pencil(topo, dims, (1,)),
                             Pencil(topo, dims, (0,), permute=(1, 0, 2)), 0,
                             kw.pop("esz", 8), (), **kw)


def _all_scaled_calls(p, scalar=F64, alpha=0.5, n=3):
    ptrs = [FAKE * (c + 2) for c in range(n)]
    return [lambda: p.pack_split_scaled(n, scalar, alpha, FAKE),
            lambda: p.local_split_scaled(scalar, alpha, FAKE, ptrs),
            lambda: p.local_join_scaled(scalar, alpha, ptrs, FAKE),
            lambda: p.unpack_join_scaled(n, scalar, alpha, FAKE),
            lambda: p.execute_split_scaled(scalar, alpha, FAKE, ptrs),
            lambda: p.execute_join_scaled(scalar, alpha, ptrs, FAKE)]


def _set_scale():
    p = _slab()
    p.set_scale(F64, 0.5)
    return p


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("make,msg", [
    (lambda: _slab(aliased=True),
     "PA_PLAN_ALIASED plan: the two sides have different element sizes"),
    (lambda: _slab(keep=((4, 0), (3, 0), (4, 0))), "keep plan"),
    (lambda: _slab(wire=native.WIRE_F64_F32), "wire plan"),
    (_set_scale, "plan with a scale set"),
    (lambda: _slab(ncomp=3), "needs a scalar plan: this one has ncomp = 3"),
    (lambda: _slab(esz=2), "invalid scalar_size 2"),
], ids=["aliased", "keep", "wire", "scale", "composite", "int16"])
def test_scaled_calls_refuse_plan_kinds(make, msg, alpha):
    """With the messages of the unscaled calls."""
    p = make()
    for call in _all_scaled_calls(p, alpha=alpha):
        with pytest.raises(RuntimeError, match=msg):
            call()


def _staged(**kw):
    """A plan whose staging is set (to addresses never touched), so that a
    call gets as far as the check of its scale."""
    p = _slab(**kw)
    p.set_buffers(FAKE * 64, FAKE * 128)
    return p


@pytest.mark.parametrize("esz,scalar,alpha,msg", [
    (16, F32, 0.5, "16-byte scalar is neither one nor two of the 4-byte"),
    (4, F64, 0.5, "4-byte scalar is neither one nor two of the 8-byte"),
    (8, 0, 0.5, "unknown scalar type 0"),
    (8, 3, 0.5, "unknown scalar type 3"),
    (8, F64, float("nan"), "alpha must be finite"),
    (8, F32, float("inf"), "alpha must be finite"),
    (8, F64, float("-inf"), "alpha must be finite"),
], ids=["16xF32", "4xF64", "code0", "code3", "nan", "inf", "-inf"])
def test_scaled_calls_refuse_a_bad_scale(esz, scalar, alpha, msg):
    p = _staged(esz=esz)
    for call in _all_scaled_calls(p, scalar, alpha):
        with pytest.raises(RuntimeError, match=msg):
            call()
    # the standalone copy refuses the same before it looks at a pointer
    lin = ((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16)
    for d in (native.SOA_SPLIT, native.SOA_JOIN):
        with pytest.raises(RuntimeError, match=msg):
            native.device_copy_soa_scale(lin, esz, 3, d, scalar, alpha, 0,
                                         [0, 0, 0])


def test_scaled_calls_refuse_bad_arguments():
    p = _slab()
    with pytest.raises(RuntimeError, match="n must be >= 2"):
        p.pack_split_scaled(1, F64, 0.5, FAKE)
    with pytest.raises(RuntimeError, match="n must be >= 2"):
        p.execute_join_scaled(F64, 0.5, [FAKE], FAKE)
    with pytest.raises(RuntimeError, match="null vector-valued array"):
        p.pack_split_scaled(3, F64, 0.5, 0)
    with pytest.raises(RuntimeError, match="null vector-valued array"):
        p.execute_split_scaled(F64, 0.5, 0, [FAKE] * 3)
    with pytest.raises(RuntimeError, match="null vector-valued array"):
        p.execute_join_scaled(F64, 0.5, [FAKE] * 3, 0)
    with pytest.raises(RuntimeError, match="null pointer for field 1"):
        p.local_split_scaled(F64, 0.5, FAKE, [8192, 0, 8192])
    with pytest.raises(RuntimeError, match="null pointer for field 2"):
        p.local_join_scaled(F64, 0.5, [8192, 8192, 0], FAKE)
    # staging must have been set, with the n-field sizes
    with pytest.raises(RuntimeError, match="pa_plan_buffer_sizes_many"):
        p.pack_split_scaled(3, F64, 0.5, FAKE)
    with pytest.raises(RuntimeError, match="pa_plan_buffer_sizes_many"):
        p.unpack_join_scaled(3, F64, 0.5, FAKE)
    # the standalone copy
    lin = ((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16)
    with pytest.raises(RuntimeError, match="n must be >= 2"):
        native.device_copy_soa_scale(lin, 8, 1, 0, F64, 0.5, 0, [0])
    with pytest.raises(RuntimeError, match="invalid scalar_size 2"):
        native.device_copy_soa_scale(lin, 2, 3, 0, F64, 0.5, 0, [0] * 3)
    with pytest.raises(RuntimeError, match="unknown direction 2"):
        native.device_copy_soa_scale(lin, 8, 3, 2, F64, 0.5, 0, [0] * 3)
    with pytest.raises(RuntimeError, match="null pointer"):
        native.device_copy_soa_scale(lin, 8, 3, 0, F64, 0.5, 0, [0] * 3)


def test_selection_query_is_unchanged():
    """Five descriptors against the values the query gave before the scaled
    calls existed (hard-coded): they select nothing of their own."""
    S, J = native.SOA_SPLIT, native.SOA_JOIN
    lin = ((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16)
    perm = ((40, 3, 50), (1, 2000, 40), 0, (150, 50, 1), 0)
    q = native.copy_kernel_kind_soa
    assert q(lin, 4, 3, S, 4096, [8192, 12288, 16384]) == (16, 4, 0, 0, 1)
    assert q(lin, 4, 3, J, 4096 + 8, [8192, 12288, 16384]) == \
        (16, 2, 0, 0, 1)
    assert q(perm, 8, 3, J, 4096 + 8, [8192 + 8] * 3) == (17, 1, 64, 16, 1)
    assert q(perm, 4, 2, S, 4096, [8192] * 2) == (17, 1, 128, 16, 1)
    assert q(lin, 8, 5, S) == (18, 1, 0, 0, 1)


# ---- 9. Python validation ---------------------------------------------------

def _pair(dtype):
    topo = Topology((1, 1))
    dims = (6, 5, 4)
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    a = PencilArray.empty(Pi, 0, dtype, elem_dims=(3,))
    fs = [PencilArray.empty(Po, 0, dtype) for _ in range(3)]
    return a, fs


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_python_refuses_a_scale_on_integer_arrays(dtype):
    a, fs = _pair(dtype)
    SplitTransposition(fs, a)              # without a scale they are fine
    JoinTransposition(a, fs, scale=None)
    for bad in (0.5, 1.0):
        with pytest.raises(ValueError, match="scale needs arrays of float32"):
            SplitTransposition(fs, a, scale=bad)
        with pytest.raises(ValueError, match="scale needs arrays of float32"):
            JoinTransposition(a, fs, scale=bad)
        with pytest.raises(ValueError, match="scale needs arrays of float32"):
            transpose_split_into(fs, a, scale=bad)
        with pytest.raises(ValueError, match="scale needs arrays of float32"):
            transpose_join_into(a, fs, scale=bad)
    with pytest.raises(ValueError, match="scale needs arrays of float32"):
        run_transpose_sim_split([fs], [a], scale=0.5)
    with pytest.raises(ValueError, match="scale needs arrays of float32"):
        run_transpose_sim_join([a], [fs], scale=0.5)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_python_refuses_a_scale_that_is_not_finite(bad):
    a, fs = _pair(np.float64)
    with pytest.raises(ValueError, match="scale must be finite"):
        SplitTransposition(fs, a, scale=bad)
    with pytest.raises(ValueError, match="scale must be finite"):
        JoinTransposition(a, fs, scale=bad)
    with pytest.raises(ValueError, match="scale must be finite"):
        run_transpose_sim_split([fs], [a], scale=bad)
    with pytest.raises(ValueError, match="scale must be finite"):
        run_transpose_sim_join([a], [fs], scale=bad)
