"""Scaled split and join transposes on one MI355X.

- pa_device_copy_soa_scale in both directions: the special values, linear
  windows at every vector width and misalignment, the tile at the tile edges,
  the generic kernel;
- the *_scaled stage calls as a multi-rank run on ONE GPU (device slice copies
  at the pa_plan_peer_message ranges standing in for the exchange), against
  the C oracle per component on the reference-scaled copies; a join's staging
  byte-identical to the unscaled n-field host run, a split's equal to the
  n-field host run on the scaled copies;
- SplitTransposition / JoinTransposition with a scale, end to end in world 1;
- launch geometry: a workgroup count past the gridDim.x limit and a window
  past byte 2^32 of the vector-valued side.

The multiply's reference is numpy on the real view (scale_util.ref_scale).
Every case asserts the selection through pa_copy_kernel_kind_soa with the real
pointers before it launches: the scaled calls select nothing of their own.
Destinations and staging are 0xAB-filled with 256-byte guards and whole
buffers are compared as bit patterns, NaN for NaN-ness.
"""

import math

import numpy as np
import pytest

from scale_util import ALPHAS, specials
from soa_scale_util import (
    KINDS, pick_alpha, same, scale_bytes, scaled_join_case, scaled_split_case,
)
from soa_util import desc_extent, ref_copy_soa, split_case
from pencilarrays_amd import (
    JoinTransposition, Pencil, PencilArray, SplitTransposition, Topology,
    build_plan,
)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import (  # noqa: E402
    check_far_sentinel, host_random, max_x, roundup,
)
from pencilarrays_amd import native  # noqa: E402
from test_gpu_soa import (  # noqa: E402
    DEV, GUARD, LIN, LINEAR_CASES, SENT, STAGE_CFGS, _dev, _e2e_cfg, _edge_kind,
    _edges, _exchange, _host_staging, _sentinel, _tile_desc, _tile_shape,
    _world1,
)

SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN
LINEAR, TILE, GENERIC = (native.KERNEL_SOA_LINEAR, native.KERNEL_SOA_TILE,
                         native.KERNEL_SOA_GENERIC)
DIRS = pytest.mark.parametrize("direction", [SPLIT, JOIN],
                               ids=["split", "join"])
KIND_IDS = sorted(KINDS)
TORCH = {"f32": torch.float32, "f64": torch.float64, "c64": torch.complex64,
         "c128": torch.complex128}


def run_copy(desc, kind, n, direction, want, alpha, seed=1, aos_lead=0,
             field_leads=None, values=None):
    """One pa_device_copy_soa_scale.  ``want``: the (kind, V) the plain query
    must report for the real pointers (V None = any).  ``aos_lead`` /
    ``field_leads[c]``: scalars by which a base pointer sits into its
    allocation.  ``values``: real scalars to tile the source with instead of
    random bytes.  The reference is ``ref_copy_soa`` on the reference-scaled
    source bytes; every buffer is compared whole, guard included, and the
    source must come through untouched.  Returns the query's answer."""
    dims, sstr, soff, dstr, doff = desc
    _, ssz, R, code = KINDS[kind]
    split = direction == SPLIT
    leads = list(field_leads or [0] * n)
    a_side, f_side = ((sstr, soff), (dstr, doff)) if split else \
        ((dstr, doff), (sstr, soff))
    a_bytes = desc_extent(dims, *a_side) * n * ssz
    f_bytes = desc_extent(dims, *f_side) * ssz

    def source(nbytes, sd):
        if values is None:
            return host_random(nbytes, sd)
        reps = -(-nbytes // values.nbytes)
        return np.tile(values, reps).view(np.uint8)[:nbytes].copy()

    if split:
        aos_h = source(a_bytes, seed)
        fld_h = [np.full(f_bytes + GUARD, SENT, np.uint8) for _ in range(n)]
    else:
        aos_h = np.full(a_bytes + GUARD, SENT, np.uint8)
        fld_h = [source(f_bytes, seed + 1 + c) for c in range(n)]
    aos_t = torch.empty(aos_lead * ssz + aos_h.size, dtype=torch.uint8,
                        device=DEV)[aos_lead * ssz:]
    aos_t.copy_(torch.from_numpy(aos_h))
    fld_t = []
    for c in range(n):
        t = torch.empty(leads[c] * ssz + fld_h[c].size, dtype=torch.uint8,
                        device=DEV)[leads[c] * ssz:]
        t.copy_(torch.from_numpy(fld_h[c]))
        fld_t.append(t)
    # the reference: the plain copy of the reference-scaled source
    if split:
        exp_a = aos_h
        exp_f = fld_h
        ref_copy_soa(desc, scale_bytes(aos_h, kind, alpha), exp_f, ssz, n,
                     True)
    else:
        exp_a, exp_f = aos_h, fld_h
        ref_copy_soa(desc, exp_a, [scale_bytes(x, kind, alpha)
                                   for x in fld_h], ssz, n, False)
    ptrs = [t.data_ptr() for t in fld_t]
    k = native.copy_kernel_kind_soa(desc, ssz, n, direction,
                                    aos_t.data_ptr(), ptrs)
    what = f"{kind} n={n} dir={direction} alpha={alpha} {desc} {k}"
    assert k.kind == want[0], what
    if want[1] is not None:
        assert k.vec == want[1], what
    native.device_copy_soa_scale(desc, ssz, n, direction, code, alpha,
                                 aos_t.data_ptr(), ptrs)
    torch.cuda.synchronize()
    got_a = aos_t.cpu().numpy()
    got_f = [t.cpu().numpy() for t in fld_t]
    if split:   # source untouched, byte for byte
        assert got_a.tobytes() == exp_a.tobytes(), what + " aos"
        for c in range(n):
            same(got_f[c], exp_f[c], kind, what + f" field {c}")
    else:
        same(got_a, exp_a, kind, what + " aos")
        for c in range(n):
            assert got_f[c].tobytes() == exp_f[c].tobytes(), \
                what + f" field {c}"
    return k


# ---- 1. the special values ---------------------------------------------------

@DIRS
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_specials_every_alpha(kind, n, direction):
    _, ssz, R, _ = KINDS[kind]
    sp = specials(R)
    L = 2 * len(sp) + 3    # every special in every component and lane
    for alpha in ALPHAS:
        k = run_copy(((L,), (1,), 0, (1,), 0), kind, n, direction,
                     (LINEAR, None), alpha, values=sp)
        assert k.vec == 1   # L is odd


# ---- 2. linear windows -------------------------------------------------------

@DIRS
@pytest.mark.parametrize("case", sorted(LINEAR_CASES))
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_linear_every_width_and_misalignment(kind, case, direction):
    desc, al, fl, V4 = LINEAR_CASES[case]
    V = V4 if kind == "f32" else min(V4, 2)
    i = sorted(LINEAR_CASES).index(case)
    run_copy(desc, kind, 3, direction, (LINEAR, V), pick_alpha(i),
             aos_lead=al, field_leads=fl)


@DIRS
@pytest.mark.parametrize("kind,n,V", [
    ("f64", 2, 2), ("f64", 4, 2), ("f32", 2, 4), ("f32", 4, 4),
    ("c64", 2, 2), ("c64", 3, 2), ("c64", 4, 2),
    ("c128", 2, 1), ("c128", 3, 1), ("c128", 4, 1),
], ids=lambda v: str(v))
def test_linear_other_pairs_and_n(kind, n, V, direction):
    run_copy(LIN, kind, n, direction, (LINEAR, V), 1.0 / 3.0)


# ---- 3. the tile at its edges ------------------------------------------------

@DIRS
@pytest.mark.parametrize("windowed", [False, True], ids=["dense", "window"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_tile_f64_at_every_edge(n, windowed, direction):
    ti, tj = _tile_shape(8, n, direction)
    assert tj == 16
    i = 0
    for e0 in _edges(ti):
        for e1 in _edges(tj):
            want = (_edge_kind(e0, e1, windowed), None)
            k = run_copy(_tile_desc(e0, e1, windowed), "f64", n, direction,
                         want, pick_alpha(i), seed=e0 * 1000 + e1)
            i += 1
            if k.kind == TILE and e0 > 1 and e1 > 1:
                assert (k.tile_i, k.tile_j) == (ti, tj)


@DIRS
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("kind", ["f32", "c64", "c128"])
def test_tile_other_pairs_corner(kind, n, direction):
    ti, tj = _tile_shape(KINDS[kind][1], n, direction)
    i = 0
    for e0 in (ti - 1, ti + 1):
        for e1 in (tj - 1, tj + 1):
            for windowed in (False, True):
                run_copy(_tile_desc(e0, e1, windowed), kind, n, direction,
                         (TILE, 1), pick_alpha(i), seed=e0 * 1000 + e1)
                i += 1


# ---- 4. the generic kernel ---------------------------------------------------

@DIRS
@pytest.mark.parametrize("kind", ["c64", "f64"])
@pytest.mark.parametrize("n,desc", [
    (5, LIN),                                   # n = 5, linear
    (5, _tile_desc(37, 21, True)),              # n = 5, permuted
    (3, ((8, 9), (2, 16), 1, (1, 8), 2)),       # no contiguous source axis
    (3, ((8, 9), (3, 24), 0, (9, 1), 0)),
], ids=lambda v: str(v).replace(" ", ""))
def test_generic(kind, n, desc, direction):
    run_copy(desc, kind, n, direction, (GENERIC, 1), 1.0 / 3.0)


def test_empty_descriptor_launches_nothing():
    d = ((0, 4), (1, 8), 0, (1, 8), 0)
    a = _sentinel(64)
    f = [_sentinel(64) for _ in range(3)]
    ptrs = [t.data_ptr() for t in f]
    for direction in (SPLIT, JOIN):
        assert native.copy_kernel_kind_soa(d, 8, 3, direction, a.data_ptr(),
                                           ptrs).kind == native.KERNEL_NONE
        native.device_copy_soa_scale(d, 8, 3, direction, native.SCALAR_F64,
                                     0.5, a.data_ptr(), ptrs)
    torch.cuda.synchronize()
    for t in [a] + f:
        assert bool((t == SENT).all())


# ---- 5. the stage API: every rank of a grid on one GPU -----------------------

def run_stage(cfg, kind, n, direction, alpha, oracle_lib_path, check=None):
    """All ranks of ``cfg`` on one GPU through the scaled split or join stages
    and the ordinary n-field stages of the other side."""
    dims, pdims, di, pi, do, po, extra = cfg
    _, ssz, R, code = KINDS[kind]
    split = direction == SPLIT
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    if split:
        aos, scaled, exp_c = scaled_split_case(cfg, kind, n, alpha,
                                               oracle_lib_path)
        staged = scaled      # staging holds the scaled scalars
    else:
        comps, scaled, exp_c, exp_aos = scaled_join_case(
            cfg, kind, n, alpha, oracle_lib_path)
        staged = comps       # staging holds the unscaled bytes
    ref = _host_staging(cfg, ssz, staged, [[len(x) for x in row]
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
            p.pack_split_scaled(n, code, alpha, ap[r], stream)
        else:
            p.pack_many(fp[r], stream)
    _exchange(plans, pyplans, n, sends, recvs)
    for r, p in enumerate(plans):
        if split:
            p.local_split_scaled(code, alpha, ap[r], fp[r], stream)
            p.unpack_many(fp[r], stream)
        else:
            p.local_join_scaled(code, alpha, fp[r], ap[r], stream)
            p.unpack_join_scaled(n, code, alpha, ap[r], stream)
    torch.cuda.synchronize()

    for r in range(nr):
        if split:
            for c in range(n):
                nb = len(exp_c[c][r])
                got = f_t[r][c].cpu().numpy()
                same(got[:nb], exp_c[c][r], kind, f"rank {r} field {c}")
                assert (got[nb:] == SENT).all(), f"rank {r} field {c} guard"
        else:
            nb = len(exp_aos[r])
            got = a_t[r].cpu().numpy()
            same(got[:nb], exp_aos[r], kind, f"rank {r}")
            assert (got[nb:] == SENT).all(), f"rank {r} guard"
        for side, bufs, i in (("send", sends, 0), ("recv", recvs, 1)):
            got = bufs[r].cpu().numpy()
            nb = sizes[r][i]
            if split:
                same(got[:nb], ref[side][r], kind, f"rank {r} {side}")
            else:   # byte-identical to the unscaled run
                assert got[:nb].tobytes() == ref[side][r].tobytes(), \
                    f"rank {r} {side} staging"
            assert (got[nb:] == SENT).all(), f"rank {r} {side} guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)


@DIRS
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("ci", range(len(STAGE_CFGS)),
                         ids=lambda i: "{0}x{1}_{2}to{4}".format(
                             *STAGE_CFGS[i]))
def test_stage_api_multirank_on_one_gpu(ci, kind, n, direction,
                                        oracle_lib_path):
    run_stage(STAGE_CFGS[ci], kind, n, direction,
              pick_alpha(ci + n + KIND_IDS.index(kind)), oracle_lib_path)


@DIRS
def test_slab_with_ragged_tiles_in_every_staged_block(direction,
                                                      oracle_lib_path):
    """x-pencil -> y-pencil of a slab over 2 ranks, permuted output, f64 x 3:
    the local copy of a split and every unpack block of a join run the scaled
    tile with at least two tiles and a ragged last one along BOTH axes."""
    n, ssz, P = 3, 8, 2
    ti, tj = _tile_shape(ssz, n, direction)
    dims = (2 * (2 * ti + 3), 2 * (2 * tj + 5), 3)
    seen = []

    def check(p, aos, fields, send, recv):
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

    cfg = (dims, (P,), (1,), (0, 1, 2), (0,), (1, 0, 2), ())
    run_stage(cfg, "f64", n, direction, 1.0 / 3.0, oracle_lib_path,
              check=check)
    assert len(seen) == (P if direction == SPLIT else P * (P - 1))


# ---- 6. end to end, world 1 --------------------------------------------------

def _typed(t, kind):
    return t.view(TORCH[kind])


def _guarded(nbytes, kind):
    raw = _sentinel(nbytes)
    return raw, _typed(raw[:nbytes], kind)


@pytest.mark.parametrize("kind", ["f64", "c64"])
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "perm"])
def test_end_to_end_world1(permuted, kind, oracle_lib_path):
    n = 3
    ssz = KINDS[kind][1]
    Pi, Po = _world1(permuted)
    cfg = _e2e_cfg(permuted)
    alpha = 1.0 / math.prod(cfg[0])
    aos, _, exp = scaled_split_case(cfg, kind, n, alpha, oracle_lib_path)
    src = PencilArray(Pi, 0, _typed(_dev(aos[0]), kind), (), (n,))
    raws, dsts = [], []
    for c in range(n):
        raw, v = _guarded(len(exp[c][0]), kind)
        raws.append(raw)
        dsts.append(PencilArray(Po, 0, v))
    d = native.NativePlan(Pi, Po, 0, ssz).copydesc_many(n, 0, 0)
    k = native.copy_kernel_kind_soa(d, ssz, n, SPLIT, src.data.data_ptr(),
                                    [x.data.data_ptr() for x in dsts])
    assert k.kind == (TILE if permuted else LINEAR)
    t = SplitTransposition(dsts, src, scale=alpha)
    t.execute(sync=False)   # deferred wait
    t.wait()
    for c in range(n):
        got = raws[c].cpu().numpy()
        nb = len(exp[c][0])
        same(got[:nb], exp[c][0], kind, c)
        assert (got[nb:] == SENT).all()
    # a scaled join against the oracle
    fields, _, _, exp_a = scaled_join_case(cfg, kind, n, alpha,
                                           oracle_lib_path)
    srcs = [PencilArray(Pi, 0, _typed(_dev(fields[c][0]), kind))
            for c in range(n)]
    raw_d, vd = _guarded(len(exp_a[0]), kind)
    j = JoinTransposition(PencilArray(Po, 0, vd, (), (n,)), srcs,
                          scale=alpha)
    j.execute(sync=False)
    j.wait()
    got = raw_d.cpu().numpy()
    same(got[:len(exp_a[0])], exp_a[0], kind, "join")
    assert (got[len(exp_a[0]):] == SENT).all()


def _unit_values(nbytes, R, seed):
    rng = np.random.default_rng(seed)
    return (1.0 + rng.random(nbytes // R.itemsize)).astype(R).view(np.uint8)


def test_split_half_join_twice_round_trip(oracle_lib_path):
    """Values in [1, 2): split by 0.5, join by 2.0, the source returns."""
    n, kind = 3, "f64"
    _, ssz, R, _ = KINDS[kind]
    Pi, Po = _world1(True)
    aos, _, exp = split_case(_e2e_cfg(True), ssz, n, oracle_lib_path)
    vals = _unit_values(len(aos[0]), R, 5)
    src = PencilArray(Pi, 0, _typed(_dev(vals), kind), (), (n,))
    dsts = [PencilArray(Po, 0, _guarded(len(exp[c][0]), kind)[1])
            for c in range(n)]
    raw_b, vb = _guarded(len(vals), kind)
    back = PencilArray(Pi, 0, vb, (), (n,))
    SplitTransposition(dsts, src, scale=0.5).execute()
    assert bool((dsts[0].data < 1).all())
    JoinTransposition(back, dsts, scale=2.0).execute()
    got = raw_b.cpu().numpy()
    assert got[:len(vals)].tobytes() == vals.tobytes()
    assert (got[len(vals):] == SENT).all()


def test_alpha_changes_between_calls_without_allocation(oracle_lib_path):
    """Two alphas on ONE native plan: no table built, nothing allocated, and
    each call's result is its own alpha's."""
    n, kind = 3, "f64"
    _, ssz, R, code = KINDS[kind]
    Pi, Po = _world1(True)
    cfg = _e2e_cfg(True)
    alphas = (1.0 / 3.0, -2.0)
    cases = [scaled_split_case(cfg, kind, n, a, oracle_lib_path)
             for a in alphas]
    src = PencilArray(Pi, 0, _typed(_dev(cases[0][0][0]), kind), (), (n,))
    dsts = [PencilArray(Po, 0, _guarded(len(cases[0][2][c][0]), kind)[1])
            for c in range(n)]
    t = SplitTransposition(dsts, src, scale=alphas[0])
    t.execute()
    nat = t._native.native
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [x.data.data_ptr() for x in dsts]
    builds = nat.stage_table_builds()
    a0 = torch.cuda.memory_allocated()
    c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    got = []
    for a in reversed(alphas):
        nat.execute_split_scaled(code, a, src.data.data_ptr(), ptrs, stream)
        nat.wait(stream)
        assert nat.stage_table_builds() == builds
        assert torch.cuda.memory_allocated() == a0
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == c0
        got.append([x.data.cpu().numpy() for x in dsts])
    for g, case in zip(got, reversed(cases)):
        for c in range(n):
            same(g[c], case[2][c][0], kind, c)


@DIRS
def test_alpha_one_is_the_unscaled_call(direction, oracle_lib_path):
    """alpha == 1.0 through the stage calls: the bytes of the unscaled call,
    NaN payloads of random bit patterns included."""
    n, kind = 3, "f32"
    _, ssz, R, code = KINDS[kind]
    Pi, Po = _world1(True)
    cfg = _e2e_cfg(True)
    aos, comps, exp = split_case(cfg, ssz, n, oracle_lib_path)
    assert np.isnan(aos[0].view(R)).any()
    p = native.NativePlan(Pi, Po, 0, ssz)
    sb, rb = p.buffer_sizes_many(n)
    send, recv = _sentinel(sb), _sentinel(rb)
    p.set_buffers(send.data_ptr(), recv.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if direction == SPLIT:
        a_t = _dev(aos[0])
        f_t = [_sentinel(len(exp[c][0])) for c in range(n)]
        ptrs = [t.data_ptr() for t in f_t]
        p.pack_split_scaled(n, code, 1.0, a_t.data_ptr(), stream)
        p.local_split_scaled(code, 1.0, a_t.data_ptr(), ptrs, stream)
        torch.cuda.synchronize()
        for c in range(n):
            got = f_t[c].cpu().numpy()
            assert got[:len(exp[c][0])].tobytes() == exp[c][0].tobytes(), c
            assert (got[len(exp[c][0]):] == SENT).all()
    else:
        # the join of the split's expected fields is the source again
        f_t = [_dev(exp[c][0]) for c in range(n)]
        ptrs = [t.data_ptr() for t in f_t]
        pj = native.NativePlan(Po, Pi, 0, ssz)
        pj.set_buffers(send.data_ptr(), recv.data_ptr())
        a_t = _sentinel(len(aos[0]))
        pj.local_join_scaled(code, 1.0, ptrs, a_t.data_ptr(), stream)
        pj.unpack_join_scaled(n, code, 1.0, a_t.data_ptr(), stream)
        torch.cuda.synchronize()
        got = a_t.cpu().numpy()
        assert got[:len(aos[0])].tobytes() == aos[0].tobytes()
        assert (got[len(aos[0]):] == SENT).all()
        pj.set_buffers(0, 0)
    p.set_buffers(0, 0)


# ---- 7. launch geometry ------------------------------------------------------

def test_tile_workgroups_past_the_grid_split():
    """(2, 2, B) with one workgroup per 2 x 2 batch and B past the gridDim.x
    limit of a 256-wide workgroup, split, (8, F64): the second grid row does
    real work.  Values in [1, 2) times 0.5 are exact, so the expected fields
    are built on the device."""
    ssz, n, alpha = 8, 2, 0.5
    B = max_x(256) + 5
    desc = ((2, 2, B), (1, 2, 4), 0, (2, 1, 4), 0)
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    aos = torch.rand(4 * B * n, dtype=torch.float64, device=DEV,
                     generator=g) + 1.0                     # [b][j][i][c]
    f_t = [_sentinel(4 * B * ssz) for _ in range(n)]
    ptrs = [t.data_ptr() for t in f_t]
    k = native.copy_kernel_kind_soa(desc, ssz, n, SPLIT, aos.data_ptr(), ptrs)
    assert k.kind == TILE, k
    wg = math.ceil(2 / k.tile_i) * math.ceil(2 / k.tile_j) * B
    assert wg > max_x(256)
    native.device_copy_soa_scale(desc, ssz, n, SPLIT, native.SCALAR_F64,
                                 alpha, aos.data_ptr(), ptrs)
    torch.cuda.synchronize()
    for c in range(n):
        exp = (aos.view(B, 2, 2, n)[..., c].transpose(1, 2) * alpha) \
            .contiguous().view(-1).view(torch.uint8)        # [b][i][j]
        assert torch.equal(f_t[c][:exp.numel()], exp), c
        assert bool((f_t[c][exp.numel():] == SENT).all())
        del exp


def test_window_past_2e32_bytes_on_the_vector_side():
    """A (70, 66, 3) permuted window whose offset on the vector-valued side
    lies past byte 2^32: the destination of a scaled join, (8, F64)."""
    kind, ssz, n, alpha = "f64", 8, 3, 1.0 / 3.0
    dims = (70, 66, 3)
    far_off = roundup((1 << 32) // (n * ssz) + 1, 8)
    a_str, f_str, f_off = (68, 1, 68 * 70 + 8), (1, 72, 72 * 66 + 8), 8
    desc = (dims, f_str, f_off, a_str, far_off)
    span = desc_extent(dims, a_str, 0)            # elements of the window
    assert far_off * n * ssz > 1 << 32
    a_bytes = (far_off + span) * n * ssz
    f_bytes = desc_extent(dims, f_str, f_off) * ssz
    lo = far_off * n * ssz
    huge = torch.empty(a_bytes + GUARD, dtype=torch.uint8, device=DEV)
    try:
        local = (dims, f_str, f_off, a_str, 0)
        win_h = np.full(span * n * ssz + GUARD, SENT, np.uint8)
        fld_h = [host_random(f_bytes, 92 + c) for c in range(n)]
        huge.fill_(SENT)
        f_t = [_dev(x) for x in fld_h]
        ref_copy_soa(local, win_h, [scale_bytes(x, kind, alpha)
                                    for x in fld_h], ssz, n, False)
        ptrs = [t.data_ptr() for t in f_t]
        k = native.copy_kernel_kind_soa(desc, ssz, n, JOIN, huge.data_ptr(),
                                        ptrs)
        assert k.kind == TILE, k
        native.device_copy_soa_scale(desc, ssz, n, JOIN, native.SCALAR_F64,
                                     alpha, huge.data_ptr(), ptrs)
        torch.cuda.synchronize()
        same(huge[lo:].cpu().numpy(), win_h, kind, "window")
        check_far_sentinel(huge, [(lo, huge.numel() - lo)])
    finally:
        huge = None
        torch.cuda.empty_cache()
