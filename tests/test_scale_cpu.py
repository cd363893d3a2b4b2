"""Scaled transposes (dest = alpha * T(src)), host only: the multiply of the
numpy mirror against numpy on the real view, the simulation against the C
oracle on the reference-scaled input, and the native plan's tables, launch
rows, selection and errors.  Expected values never come from the code under
test (scale_util)."""

import math
import os

import numpy as np
import pytest

from keep_util import CPU_CFGS, cfg_id, expected_keep, keep_sets
from pencilarrays_amd import (
    ManyPencilArray, MultiTransposition, PencilArray, Transposition, native,
    run_transpose_sim, run_transpose_sim_many, scale_array, transpose_into,
    transpose_many_into,
)
from pencilarrays_amd.scale import resolve_scale
from scale_util import (
    A, ALPHAS, F32, F64, GEN, KINDS, LIN, SCALE_KINDS, STAGES, TILE,
    assert_same, expected_rows, expected_scaled, kind_parents, oracle,
    pencils, plan_of, plan_rows, ref_scale, seeded_patterns, seeded_values,
    specials, tile_shape,
)
from util import SWEEP

ID3 = (0, 1, 2)
SENT = 0xAB
REALS = [np.float32, np.float64]


# ---- 1. the multiply ---------------------------------------------------------

@pytest.mark.parametrize("S", REALS, ids=lambda s: np.dtype(s).name)
def test_special_values(S):
    fi = np.finfo(S)
    U = {4: np.uint32, 8: np.uint64}[np.dtype(S).itemsize]

    def bits(x):
        return np.asarray(x, dtype=S).view(U)

    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=S)
    got = scale_array(x, -2.0)
    assert (bits(got[:4]) == bits([-0.0, 0.0, -np.inf, np.inf])).all()
    assert np.isnan(got[4])
    got = scale_array(x, 0.0)  # inf * 0 is NaN, -0 * 0 is -0
    assert (bits(got[:2]) == bits([0.0, -0.0])).all()
    assert np.isnan(got[2:]).all()
    assert np.isinf(scale_array(np.array([fi.max], dtype=S), 2.0)[0])
    half = scale_array(np.array([fi.tiny], dtype=S), 0.5)
    assert half[0] > 0 and half[0] < fi.tiny           # a subnormal, kept
    assert bits(half)[0] == U(1) << U(fi.nmant - 1)
    # odd subnormals x 0.5 tie: to even
    odd = np.array([1, 3, 5, 7], dtype=U).view(S)
    assert (bits(scale_array(odd, 0.5)) == [0, 2, 2, 4]).all()
    # values x 1/3: one rounding of the product with S(1/3)
    v = np.array([1.0, 3.0, 10.0, -7.0, fi.max, fi.tiny], dtype=S)
    with np.errstate(all="ignore"):
        assert (bits(scale_array(v, 1 / 3)) == bits(v * S(1 / 3))).all()
    assert float(scale_array(np.array([3.0], dtype=S), 1 / 3)[0]) == \
        float(S(3.0) * S(1 / 3))


@pytest.mark.parametrize("alpha", ALPHAS, ids=repr)
@pytest.mark.parametrize("S", REALS, ids=lambda s: np.dtype(s).name)
def test_alphas_on_specials_and_patterns(S, alpha):
    a = np.dtype(S).type(alpha)
    assert a == np.float32(alpha) if S is np.float32 else a == alpha
    if alpha == 1e-320:
        assert (a == 0) == (S is np.float32)
    sc = resolve_scale(S, alpha)
    assert sc.a.dtype == np.dtype(S) and sc.a.tobytes() == a.tobytes()
    x = np.concatenate([specials(S), seeded_patterns(100_000, S, 0x5EED)])
    with np.errstate(all="ignore"):
        want = x * a
    assert want.dtype == np.dtype(S)
    assert_same(scale_array(x, alpha), want, f"{alpha}")
    # a complex item is two scalars, not a complex multiply
    C = {np.float32: np.complex64, np.float64: np.complex128}[S]
    z = x[:len(x) // 2 * 2].view(C)
    assert_same(scale_array(z, alpha), want[:len(z) * 2].view(C))
    assert_same(ref_scale(z, alpha), want[:len(z) * 2].view(C))


# ---- 2. the simulation against the C oracle ----------------------------------

def _arrays(P, parents_f, kind, extra):
    dtype, elem = KINDS[kind][:2]
    return [PencilArray(P, r, parents_f[r].copy(), extra, elem)
            for r in range(len(parents_f))]


def _sentinels(P, exp_f, kind, extra):
    dtype, elem = KINDS[kind][:2]
    return [PencilArray(P, r, np.full(exp_f[r].nbytes, SENT, np.uint8)
                        .view(dtype), extra, elem)
            for r in range(len(exp_f))]


SIM_CFGS = sorted({c[:7] for c in SWEEP}, key=repr)


@pytest.mark.parametrize("kind", ["f32", "f64", "c64", "c128", "3xf64"])
@pytest.mark.parametrize("cfg", SIM_CFGS, ids=cfg_id)
def test_simulation_equals_oracle_on_scaled_input(cfg, kind, oracle_lib_path):
    alpha = 1.0 / (130 * 67 * 35)
    Pi, Po = pencils(cfg)
    extra = cfg[6]
    nr = math.prod(cfg[1])
    n = 3
    parents = kind_parents(kind, cfg, n, oracle_lib_path)
    exp = expected_scaled(kind, parents, cfg, alpha, oracle_lib_path)
    # one field; every rank's send buffer is that of the unscaled run
    srcs = _arrays(Pi, parents[0], kind, extra)
    dsts = _sentinels(Po, exp[0], kind, extra)
    plain = _sentinels(Po, exp[0], kind, extra)
    st, st0 = {}, {}
    run_transpose_sim(dsts, srcs, st, scale=alpha)
    run_transpose_sim(plain, srcs, st0)
    for r in range(nr):
        assert_same(dsts[r].data, exp[0][r], f"rank {r}")
        assert st["send"][r].view(np.uint8).tobytes() == \
            st0["send"][r].view(np.uint8).tobytes(), r
    # three fields, one message per peer
    srcs = [_arrays(Pi, parents[f], kind, extra) for f in range(n)]
    dsts = [_sentinels(Po, exp[f], kind, extra) for f in range(n)]
    plain = [_sentinels(Po, exp[f], kind, extra) for f in range(n)]
    st, st0 = {}, {}
    by_rank = lambda x: [[x[f][r] for f in range(n)] for r in range(nr)]
    run_transpose_sim_many(by_rank(dsts), by_rank(srcs), st, scale=alpha)
    run_transpose_sim_many(by_rank(plain), by_rank(srcs), st0)
    for r in range(nr):
        for f in range(n):
            assert_same(dsts[f][r].data, exp[f][r], f"field {f} rank {r}")
        assert st["send"][r].view(np.uint8).tobytes() == \
            st0["send"][r].view(np.uint8).tobytes(), r


@pytest.mark.parametrize("alpha", ALPHAS, ids=repr)
def test_simulation_every_alpha(alpha, oracle_lib_path):
    cfg = SWEEP[0][:7]
    Pi, Po = pencils(cfg)
    for kind in ("f32", "c128"):
        parents = kind_parents(kind, cfg, 1, oracle_lib_path)
        exp = expected_scaled(kind, parents, cfg, alpha, oracle_lib_path)
        srcs = _arrays(Pi, parents[0], kind, ())
        dsts = _sentinels(Po, exp[0], kind, ())
        run_transpose_sim(dsts, srcs, scale=alpha)
        for r in range(4):
            assert_same(dsts[r].data, exp[0][r], f"{kind} rank {r}")


KEEP_CASES = [(c, k) for c in CPU_CFGS
              for k in ("inside", "two_ranges", "nothing", "full")]


@pytest.mark.parametrize("kind", ["f64", "c64"])
@pytest.mark.parametrize("cfg,kname", KEEP_CASES,
                         ids=lambda v: v if isinstance(v, str) else cfg_id(v))
def test_keep_with_scale_equals_masked_scaled_oracle(cfg, kname, kind,
                                                     oracle_lib_path):
    alpha = 1.0 / 3.0
    keep = keep_sets(cfg)[kname]
    dtype, elem, S, code, nscal = KINDS[kind]
    esz = np.dtype(S).itemsize * nscal
    Pi, Po = pencils(cfg)
    nr = math.prod(cfg[1])
    parents = kind_parents(kind, cfg, 1, oracle_lib_path)
    scaled = [[ref_scale(p, alpha).view(np.uint8) for p in parents[0]]]
    for fill, zero in (("zero", True), (None, False)):
        exp = expected_keep(scaled, cfg, esz, keep, oracle_lib_path,
                            fill_zero=zero, sentinel=SENT)[0]
        srcs = _arrays(Pi, parents[0], kind, cfg[6])
        dsts = _sentinels(Po, [e.view(dtype) for e in exp], kind, cfg[6])
        run_transpose_sim(dsts, srcs, keep=keep, fill=fill, scale=alpha)
        for r in range(nr):
            assert_same(dsts[r].data, exp[r].view(dtype), f"{fill} rank {r}")


def test_inplace_chain_scales_twice():
    cfg = ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    Pi, Po = pencils(cfg)
    alpha = 1.0 / 3.0
    ms = [ManyPencilArray((Pi, Po), r) for r in range(4)]
    orig = []
    for r, m in enumerate(ms):
        m.first.data[:] = seeded_values(Pi.length_local(r), np.float64, 40 + r)
        orig.append(m.first.data.copy())
    run_transpose_sim([m[1] for m in ms], [m[0] for m in ms], scale=alpha)
    run_transpose_sim([m[0] for m in ms], [m[1] for m in ms], scale=alpha)
    for r, m in enumerate(ms):
        assert_same(m.first.data, ref_scale(ref_scale(orig[r], alpha), alpha),
                    f"rank {r}")


def _gloo_worker(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        repo = os.path.dirname(here)
        for p in (repo, os.path.join(repo, "oracle"), here):
            sys.path.insert(0, p)
        from conftest import ensure_oracle_lib
        import scale_util as su
        cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        lib = ensure_oracle_lib()
        Pi, Po = su.pencils(cfg)
        for kind, alpha in (("f64", 1 / 3), ("c64", -2.0)):
            parents = su.kind_parents(kind, cfg, 1, lib)
            exp = su.expected_scaled(kind, parents, cfg, alpha, lib)[0]
            dtype = su.KINDS[kind][0]
            src = PencilArray(Pi, rank, parents[0][rank].copy())
            dst = PencilArray(Po, rank, np.full(exp[rank].nbytes, 0xAB,
                                                np.uint8).view(dtype))
            Transposition(dst, src, scale=alpha).execute()
            su.assert_same(dst.data, exp[rank], f"{kind} rank {rank}")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2_scale():
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, 29900 + os.getpid() % 90), nprocs=2,
             join=True)


# ---- 3. native plan: tables and rows ------------------------------------------

ROW_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, (3,)),
]
SLAB = ((64, 64, 64), (8,), (1,), ID3, (0,), (1, 0, 2), ())
VARIANTS = ["plain", "aliased", "keep"]


def _variant(cfg, v):
    if v == "keep":
        return dict(keep=keep_sets(cfg[:6] + ((),))["two_dims"])
    return dict(aliased=(v == "aliased"))


@pytest.mark.parametrize("kind", ["f64", "c64", "3xf64"])
@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("cfg", ROW_CFGS, ids=cfg_id)
def test_tables_unchanged_and_rows_are_the_partition(cfg, v, kind):
    dtype, elem, S, code, nscal = KINDS[kind]
    kw = _variant(cfg, v)
    for r in range(math.prod(cfg[1])):
        plain = plan_of(cfg, r, kind, **kw)
        p = plan_of(cfg, r, kind, alpha=0.5, **kw)
        assert plain.plan_scale() is None
        assert p.plan_scale() == (code, 0.5)
        nk = plain.nproc_sub
        for which in range(5):
            for k in range(nk if which in (1, 2) else 1):
                if v == "keep":
                    assert p.nsub(which, k) == plain.nsub(which, k)
                    for s in range(plain.nsub(which, k)):
                        assert p.copydesc_sub(3, 2, which, k, s) == \
                            plain.copydesc_sub(3, 2, which, k, s)
                else:
                    assert p.copydesc(which, k) == plain.copydesc(which, k)
                    assert p.copydesc_many(3, 2, which, k) == \
                        plain.copydesc_many(3, 2, which, k)
        assert p.buffer_sizes() == plain.buffer_sizes()
        assert p.buffer_sizes_many(3) == plain.buffer_sizes_many(3)
        if plain.r_dim >= 0:
            for k in range(nk):
                for n in (1, 3):
                    assert p.peer_message(n, k) == plain.peer_message(n, k)
        for n in (1, 3):
            got = plan_rows(p, n)
            assert got[native.STAGE_PACK] == \
                plain.stage_launches(n, native.STAGE_PACK)
            assert all(l.kind not in SCALE_KINDS
                       for l in got[native.STAGE_PACK])
            assert got == expected_rows(plain, n, code, nscal), (r, n)
            for s in (native.STAGE_LOCAL, native.STAGE_UNPACK):
                assert all(l.kind in SCALE_KINDS | {native.KERNEL_FILL}
                           for l in got[s])


def _rows(l):
    return [(x.kind, x.grouped, x.entries) for x in l]


def test_slab_launch_rows():
    n = 3
    for r in (0, 5):
        plain = plan_of(SLAB, r, "f64")
        p = plan_of(SLAB, r, "f64", alpha=1 / 3)
        tiles = (native.KERNEL_TILE, native.KERNEL_TILE_VS)
        urow = plain.stage_launches(n, native.STAGE_UNPACK)
        assert len(urow) == 1 and urow[0].kind in tiles and \
            (urow[0].grouped, urow[0].entries) == (True, 21)
        got = plan_rows(p, n)
        assert _rows(got[native.STAGE_UNPACK]) == [(TILE, True, 21)]
        assert _rows(got[native.STAGE_LOCAL]) == [(TILE, True, 3)]
        assert got[native.STAGE_PACK] == \
            plain.stage_launches(n, native.STAGE_PACK)
        # one 8 x 64 x 64 block per peer: 64 / 64 x 8 -> 1 tile x 64 batches
        ti, tj = tile_shape(F64, 1)
        per = math.ceil(64 / ti) * math.ceil(8 / tj) * 64
        assert got[native.STAGE_UNPACK][0].workgroups == 21 * per
        assert got == expected_rows(plain, n, F64, 1)


def test_misaligned_field_moves_to_a_row_of_lower_v():
    # same decomposition, no permutation: every local copy is one linear run
    cfg = ((16, 21, 41), (2, 2), (1, 2), ID3, (1, 2), ID3, ())
    n = 3
    plain = plan_of(cfg, 0, "f64")
    p = plan_of(cfg, 0, "f64", alpha=0.5)
    assert _rows(p.stage_launches(n, native.STAGE_LOCAL)) == [(LIN, True, 3)]
    dsts = [0x10000, 0x20008, 0x30000]  # field 1: one f64 into its allocation
    got = p.stage_launches(n, native.STAGE_LOCAL, None, dsts)
    assert _rows(got) == [(LIN, True, 2), (LIN, True, 1)]
    # V = 2 against V = 1: the one misaligned entry needs as many workgroups
    # as the two aligned ones together (up to the rounding of each grid)
    assert abs(got[1].workgroups - got[0].workgroups) <= 2
    assert got == expected_rows(plain, n, F64, 1, dp=dsts)[native.STAGE_LOCAL]
    # the slab without a permutation: every unpack is a window of runs
    slab_id = SLAB[:5] + (ID3, ())
    plain = plan_of(slab_id, 0, "f64")
    p = plan_of(slab_id, 0, "f64", alpha=0.5)
    assert _rows(p.stage_launches(n, native.STAGE_UNPACK)) == \
        [(LIN, True, 21)]
    got = p.stage_launches(n, native.STAGE_UNPACK, None, dsts)
    assert _rows(got) == [(LIN, True, 14), (LIN, True, 7)]
    assert got[1].workgroups == got[0].workgroups  # V = 1 against V = 2
    assert got == expected_rows(plain, n, F64, 1, dp=dsts)[native.STAGE_UNPACK]


def test_alpha_one_is_the_ordinary_plan():
    for cfg in ROW_CFGS:
        for r in range(math.prod(cfg[1])):
            plain = plan_of(cfg, r, "f64")
            p = plan_of(cfg, r, "f64", alpha=1.0)
            assert p.plan_scale() is None
            q = plan_of(cfg, r, "f64", alpha=0.5)
            q.set_scale(F64, 1.0)
            assert q.plan_scale() is None
            for s in STAGES:
                assert p.stage_launches(3, s) == plain.stage_launches(3, s)
                assert q.stage_launches(3, s) == plain.stage_launches(3, s)
            assert p.stage_table_count() == 0


# ---- 4. selection ---------------------------------------------------------------

def _lin(n0=64, n1=5, sp=64, dp=64, soff=0, doff=0):
    return ((n0, n1), (1, sp), soff, (1, dp), doff)


def _kind(desc, code, nscal=1, s=A, d=A):
    return native.copy_kernel_kind_scale(desc, code, nscal, s, d)


@pytest.mark.parametrize("code,vmax,sz", [(F32, 4, 4), (F64, 2, 8)])
def test_selection_linear(code, vmax, sz):
    assert _kind(_lin(), code) == (LIN, vmax, 0, 0, 1)
    assert _kind(((640,), (1,), 0, (1,), 0), code) == (LIN, vmax, 0, 0, 1)
    h = vmax // 2
    lowered = [
        dict(s=A + h * sz), dict(d=A + h * sz),
        dict(desc=_lin(soff=h)), dict(desc=_lin(doff=h)),
        dict(desc=_lin(sp=64 + h)), dict(desc=_lin(dp=64 + h)),
        dict(desc=_lin(n0=64 - h, sp=64, dp=64)),
    ]
    for kw in lowered:
        kw = dict(kw)
        k = _kind(kw.pop("desc", _lin()), code, **kw)
        assert (k.kind, k.vec) == (LIN, h), kw
    # one scalar off on a side: down to V = 1 (f32 from 4)
    assert _kind(_lin(), code, s=A + sz).vec == 1
    assert _kind(_lin(doff=1), code).vec == 1
    # nscal joins the run: 3 x 5 scalars per row is odd
    assert _kind(_lin(n0=5, sp=5, dp=7), code, 3).vec == 1
    assert _kind(_lin(n0=6, sp=6, dp=8), code, 2).vec == vmax


def test_selection_tile_generic_none():
    t = ((10, 7, 3), (1, 10, 70), 0, (7, 1, 70), 0)
    for code in (F32, F64):
        for nscal in (1, 2, 3, 4):
            ti, tj = tile_shape(code, nscal)
            assert _kind(t, code, nscal) == (TILE, 1, ti, tj, 1)
        assert _kind(t, code, 6) == (GEN, 1, 0, 0, 1)
        assert _kind(((10, 7), (2, 20), 0, (7, 1), 0), code) == \
            (GEN, 1, 0, 0, 1)
        assert _kind(((10, 0), (1, 10), 0, (7, 1), 0), code).kind == \
            native.KERNEL_NONE
    # ta behind the batch axis
    assert _kind(((10, 3, 7), (1, 10, 30), 0, (7, 70, 1), 0), F64).kind == TILE


# ---- 5. errors --------------------------------------------------------------------

def test_errors():
    cfg = ROW_CFGS[0]
    Pi, Po = pencils(cfg)
    wire = native.NativePlan(Pi, Po, 0, 8, wire=native.WIRE_F64_F32)
    with pytest.raises(RuntimeError, match="wire"):
        wire.set_scale(F64, 0.5)
    two = native.NativePlan(Pi, Po, 0, 2)
    with pytest.raises(RuntimeError, match="multiple"):
        two.set_scale(F32, 0.5)
    p = plan_of(cfg, 0, "f64")
    with pytest.raises(RuntimeError, match="scalar"):
        p.set_scale(3, 0.5)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError, match="finite"):
            p.set_scale(F64, bad)
    assert p.plan_scale() is None
    lib = native.load()
    I64 = native.I64
    args = (2, (I64 * 2)(4, 4), (I64 * 2)(1, 4), I64(0), (I64 * 2)(4, 1),
            I64(0), F64, I64(1), None, None)
    assert lib.pa_copy_kernel_kind_scale(*args, None) != 0
    assert b"null" in lib.pa_last_error()
    with pytest.raises(RuntimeError, match="scalar"):
        native.copy_kernel_kind_scale(_lin(), 0)
    assert lib.pa_plan_scale(None, None, None) == 0


def test_python_errors():
    cfg = ((12, 10, 8), (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
    Pi, Po = pencils(cfg)

    def pair(dtype):
        return (PencilArray.empty(Po, 0, dtype=dtype),
                PencilArray(Pi, 0, np.zeros(Pi.length_local(0), dtype=dtype)))

    for dtype in (np.int32, np.float16):
        d, s = pair(dtype)
        for call in (lambda: Transposition(d, s, scale=0.5),
                     lambda: MultiTransposition([d], [s], scale=0.5),
                     lambda: transpose_into(d, s, scale=0.5),
                     lambda: transpose_many_into([d], [s], scale=0.5),
                     lambda: run_transpose_sim([d], [s], scale=0.5)):
            with pytest.raises(ValueError, match="scale"):
                call()
    d, s = pair(np.float64)
    for call in (lambda: Transposition(d, s, scale=0.5, wire_dtype="float32"),
                 lambda: MultiTransposition([d], [s], scale=0.5,
                                            wire_dtype="float32"),
                 lambda: run_transpose_sim([d], [s], scale=0.5,
                                           wire_dtype="float32")):
        with pytest.raises(ValueError, match="wire_dtype"):
            call()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            Transposition(d, s, scale=bad)
    assert Transposition(d, s, scale=1.0).scale is None
    assert Transposition(d, s).scale is None
    t = Transposition(d, s, scale=0.25)
    assert (t.scale.code, t.scale.alpha) == (F64, 0.25)
