"""Reduced-precision wire on the host: ``round_wire`` against its references,
the numpy mirror (simulated ranks, multi-field, chains, in place, gloo)
against the C oracle run on the reference-rounded input, the native wire
plan's tables and byte counts, the converting-kernel selection, and errors.

Contract: ``dest == T(round_w(src))`` bit for bit on every non-NaN scalar,
whatever the process grid."""

import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from pencilarrays_amd import (
    ManyPencilArray, MultiTransposition, Pencil, PencilArray, Topology,
    Transposition, build_plan, native, round_wire, run_transpose_sim,
    run_transpose_sim_many, transpose_into,
)
from util import SWEEP
from wire_util import (
    ELEM_KINDS, NARROW, PAIRS, ROUND, WIDEN, assert_same, carrier,
    expected_rounded, kind_parents, ref_narrow, ref_round, seeded_patterns,
    specials,
)

KINDS = list(ELEM_KINDS)


def _ids(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}e{c[6]}"


# ---- round_wire ------------------------------------------------------------

@pytest.mark.parametrize("pair", list(PAIRS))
def test_round_wire_special_values(pair):
    x = specials(pair)
    assert_same(round_wire(x, PAIRS[pair][1]), ref_round(x, pair), pair)
    # the values the contract names, spelled out
    if pair == "f64_f32":
        r = round_wire(np.array([3.5e38, 2.0 ** -150, 1 + 2.0 ** -24,
                                 1 + 3 * 2.0 ** -24, 1e-40]), "float32")
        assert r[0] == np.inf and r[1] == 0 and r[2] == 1
        assert r[3] == 1 + 2.0 ** -22 and r[4] == float(np.float32(1e-40))
    if pair == "f32_f16":
        r = round_wire(np.array([65520, 65519.9, 2.0 ** -25], np.float32),
                       np.float16)
        assert r[0] == np.inf and r[1] == 65504 and r[2] == 0
    if pair == "f32_bf16":
        r = round_wire(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8],
                                np.float32), torch.bfloat16)
        assert r[0] == 1 and r[1] == 1 + 2.0 ** -6


@pytest.mark.parametrize("pair", list(PAIRS))
def test_round_wire_random_patterns(pair):
    x = seeded_patterns(100_000, pair, 0xB17)
    got = round_wire(x, PAIRS[pair][1])
    assert_same(got, ref_round(x, pair), pair)
    assert_same(round_wire(got, PAIRS[pair][1]), got, "idempotent")


def test_round_wire_complex_and_shape():
    x = (np.arange(12) * (1 + 2.0 ** -24)).reshape(3, 4) * (1 + 1j)
    r = round_wire(x, "float32")
    assert r.shape == x.shape and r.dtype == np.complex128
    assert_same(r, ref_round(x, "f64_f32"))


# ---- the numpy mirror against the C oracle ---------------------------------

def _pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg[:7]
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po))


def _arrays(kind, cfg, parents_f):
    dtype, elem, _, _ = ELEM_KINDS[kind]
    Pi, Po = _pencils(cfg)
    extra = cfg[6]
    nr = len(parents_f)
    srcs = [PencilArray(Pi, r, parents_f[r].copy(), extra, elem)
            for r in range(nr)]
    dsts = [PencilArray.empty(Po, r, dtype=dtype, extra_dims=extra,
                              elem_dims=elem) for r in range(nr)]
    for d in dsts:
        d.data.view(np.uint8)[:] = 0xAB
    return srcs, dsts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", SWEEP, ids=_ids)
def test_sim_matches_oracle_on_rounded_input(cfg, kind, oracle_lib_path):
    cfg = cfg[:7]
    dims, pdims, di, pi, do, po, extra = cfg
    pair = ELEM_KINDS[kind][2]
    parents = kind_parents(kind, dims, pdims, di, extra, 1, oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)
    srcs, dsts = _arrays(kind, cfg, parents[0])
    run_transpose_sim(dsts, srcs, wire_dtype=PAIRS[pair][1])
    for r in range(len(srcs)):
        assert_same(dsts[r].data, exp[0][r], f"rank {r}")
        assert srcs[r].data.tobytes() == parents[0][r].tobytes()


SEND_CFGS = [SWEEP[0], SWEEP[4], SWEEP[8], SWEEP[13], SWEEP[14]]


@pytest.mark.parametrize("kind", ["f64", "3xf64", "f32_bf16", "f32_f16"])
@pytest.mark.parametrize("cfg", SEND_CFGS, ids=_ids)
def test_send_buffers_are_narrowed_blocks_of_half_the_bytes(
        cfg, kind, oracle_lib_path):
    cfg = cfg[:7]
    dims, pdims, di, pi, do, po, extra = cfg
    pair = ELEM_KINDS[kind][2]
    stored = PAIRS[pair][0]
    parents = kind_parents(kind, dims, pdims, di, extra, 1, oracle_lib_path)
    srcs, dsts = _arrays(kind, cfg, parents[0])
    plain, wire = {}, {}
    run_transpose_sim(dsts, srcs, staging_out=plain)
    run_transpose_sim(dsts, srcs, staging_out=wire,
                      wire_dtype=PAIRS[pair][1])
    sent = 0
    for r in range(len(srcs)):
        full = np.ascontiguousarray(plain["send"][r]).view(np.uint8) \
            .view(stored)
        got = wire["send"][r]
        assert got.dtype == carrier(pair)
        assert 2 * got.nbytes == full.nbytes
        assert_same(got, ref_narrow(full, pair), f"rank {r} send")
        assert 2 * wire["recv"][r].nbytes == plain["recv"][r].nbytes
        sent += got.nbytes
    assert sent > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", [SWEEP[0], SWEEP[8], SWEEP[13]], ids=_ids)
def test_sim_many_three_fields(cfg, kind, oracle_lib_path):
    cfg = cfg[:7]
    dims, pdims, di, pi, do, po, extra = cfg
    pair = ELEM_KINDS[kind][2]
    n = 3
    parents = kind_parents(kind, dims, pdims, di, extra, n, oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)
    per_field = [_arrays(kind, cfg, parents[f]) for f in range(n)]
    nr = len(parents[0])
    srcs = [[per_field[f][0][r] for f in range(n)] for r in range(nr)]
    dsts = [[per_field[f][1][r] for f in range(n)] for r in range(nr)]
    st = {}
    run_transpose_sim_many(dsts, srcs, staging_out=st,
                           wire_dtype=PAIRS[pair][1])
    for r in range(nr):
        for f in range(n):
            assert_same(dsts[r][f].data, exp[f][r], f"rank {r} field {f}")
    plan0 = build_plan(*_pencils(cfg), 0, extra)
    nc = ELEM_KINDS[kind][3]
    assert st["send"][0].nbytes == \
        n * plan0.send_nelem_total * nc * PAIRS[pair][3]


CHAIN = ((16, 21, 41), (2, 2))


def _chain_pencils():
    dims, pdims = CHAIN
    topo = Topology(pdims)
    return (Pencil(topo, dims, (1, 2)),
            Pencil(topo, dims, (0, 2), permute=(1, 2, 0)),
            Pencil(topo, dims, (0, 1), permute=(2, 1, 0)))


@pytest.mark.parametrize("kind", ["f64", "c128", "f32_bf16"])
def test_chain_rounds_once(kind, oracle_lib_path):
    """x -> y -> z -> y -> x returns round_w(src): round_w is idempotent."""
    dims, pdims = CHAIN
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    pens = _chain_pencils()
    parents = kind_parents(kind, dims, pdims, (1, 2), (), 1,
                           oracle_lib_path)[0]
    nr = len(parents)
    cur = [PencilArray(pens[0], r, parents[r].copy()) for r in range(nr)]
    for nxt in (1, 2, 1, 0):
        out = [PencilArray.empty(pens[nxt], r, dtype=dtype)
               for r in range(nr)]
        run_transpose_sim(out, cur, wire_dtype=PAIRS[pair][1])
        cur = out
    for r in range(nr):
        assert_same(cur[r].data, ref_round(parents[r], pair), f"rank {r}")


def test_inplace_pair_over_manypencilarray(oracle_lib_path):
    """x -> y -> x in place (aliased plans: the staged self block is narrowed
    into the recv tail and widened out of it)."""
    dims, pdims = CHAIN
    pens = _chain_pencils()[:2]
    parents = kind_parents("f64", dims, pdims, (1, 2), (), 1,
                           oracle_lib_path)[0]
    nr = len(parents)
    ms = [ManyPencilArray(pens, r) for r in range(nr)]
    for r in range(nr):
        ms[r][0].data[:] = parents[r]
    run_transpose_sim([m[1] for m in ms], [m[0] for m in ms],
                      wire_dtype="float32")
    cfg = (dims, pdims, (1, 2), (0, 1, 2), (0, 2), (1, 2, 0), ())
    exp = expected_rounded("f64", [parents], cfg, oracle_lib_path)[0]
    for r in range(nr):
        assert_same(ms[r][1].data, exp[r], f"rank {r} y")
    run_transpose_sim([m[0] for m in ms], [m[1] for m in ms],
                      wire_dtype="float32")
    for r in range(nr):
        assert_same(ms[r][0].data, ref_round(parents[r], "f64_f32"),
                    f"rank {r} back")


def test_world1_execute_and_multitransposition(oracle_lib_path):
    dims = (42, 31, 29)
    cfg = (dims, (1, 1), (1, 2), (0, 1, 2), (0, 2), (1, 2, 0), ())
    parents = kind_parents("f64", dims, (1, 1), (1, 2), (), 2,
                           oracle_lib_path)
    exp = expected_rounded("f64", parents, cfg, oracle_lib_path)
    Pi, Po = _pencils(cfg)
    srcs = [PencilArray(Pi, 0, parents[f][0].copy()) for f in range(2)]
    dsts = [PencilArray.empty(Po, 0) for _ in range(2)]
    transpose_into(dsts[0], srcs[0], wire_dtype=np.float32)
    assert_same(dsts[0].data, exp[0][0])
    dsts[0].data[:] = 0
    MultiTransposition(dsts, srcs, wire_dtype=torch.float32).execute()
    for f in range(2):
        assert_same(dsts[f].data, exp[f][0], f"field {f}")


# ---- native plan, host only -------------------------------------------------

PLAN_CFGS = [
    ((16, 21, 41), (2, 2), (1, 2), (0, 1, 2), (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (8,), (1,), (0, 1, 2), (0,), (1, 0, 2), ()),
    ((3, 21, 41), (4, 2), (0, 2), (0, 1, 2), (1, 2), (0, 1, 2), (3,)),
]


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("kind", ["f64", "c128", "3xf64", "f32_bf16"])
@pytest.mark.parametrize("cfg", PLAN_CFGS, ids=_ids)
def test_native_wire_plan_tables_and_bytes(cfg, kind, aliased):
    dims, pdims, di, pi, do, po, extra = cfg
    _, _, pair, nc = ELEM_KINDS[kind]
    stored = np.dtype(PAIRS[pair][0]).itemsize
    code, wsz = PAIRS[pair][2], PAIRS[pair][3]
    Pi, Po = _pencils(cfg)
    nr = math.prod(pdims)
    plain = [native.NativePlan(Pi, Po, r, stored, extra, aliased=aliased,
                               ncomp=nc) for r in range(nr)]
    wire = [native.NativePlan(Pi, Po, r, stored, extra, aliased=aliased,
                              ncomp=nc, wire=code) for r in range(nr)]
    cvt = {native.KERNEL_CVT_LINEAR, native.KERNEL_CVT_TILE,
           native.KERNEL_CVT_GENERIC}
    for r in range(nr):
        p, w = plain[r], wire[r]
        assert w.plan_wire() == code and p.plan_wire() == 0
        P = p.nproc_sub
        for which in range(5):
            for k in range(P if which in (1, 2) else 1):
                assert w.copydesc(which, k) == p.copydesc(which, k)
                assert w.copydesc_many(3, 2, which, k) == \
                    p.copydesc_many(3, 2, which, k)
        for a, b in ((p.buffer_sizes(), w.buffer_sizes()),
                     (p.buffer_sizes_many(3), w.buffer_sizes_many(3))):
            assert [x * wsz for x in a] == [y * stored for y in b]
        py = build_plan(Pi, Po, r, extra, aliased=aliased)
        for blk in py.peers:
            for n in (1, 3):
                mp_, mw = p.peer_message(n, blk.peer_k), \
                    w.peer_message(n, blk.peer_k)
                assert [x * wsz for x in mp_] == [y * stored for y in mw]
                # what I send is what the peer receives
                back = wire[blk.global_rank].peer_message(n, py.my_k)
                assert mw[1] == back[3]
        seen = 0
        for stage in (native.STAGE_PACK, native.STAGE_LOCAL,
                      native.STAGE_UNPACK):
            rows = w.stage_launches(3, stage)
            assert all(l.kind in cvt and not l.grouped and l.entries == 1
                       and l.workgroups > 0 for l in rows), rows
            seen += len(rows)
        if py.local is not None or py.self_pack is not None or \
                any(b.pack is not None for b in py.peers):
            assert seen > 0


# ---- selection, host only ---------------------------------------------------

A = 4096  # a well-aligned fake address: never dereferenced


def _kind(desc, pair, op, nc=1, s=A, d=A):
    return native.copy_kernel_kind_wire(desc, PAIRS[pair][2], op, nc, s, d)


def _sizes(pair, op):
    stored = np.dtype(PAIRS[pair][0]).itemsize
    w = PAIRS[pair][3]
    return (w if op == WIDEN else stored), (w if op == NARROW else stored)


@pytest.mark.parametrize("op", [NARROW, WIDEN, ROUND])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_selection_linear_vector_width(pair, op):
    ss, ds = _sizes(pair, op)
    V = 16 // max(ss, ds)
    assert V == (2 if pair == "f64_f32" else 4)
    full = ((64, 5), (1, 80), 8, (1, 64), 16)
    k = _kind(full, pair, op)
    assert k == (native.KERNEL_CVT_LINEAR, V, 0, 0, 1)
    assert _kind(((640,), (1,), 0, (1,), 0), pair, op).vec == V  # 1-D
    # one rule broken at a time lowers V: each to the next power of two the
    # broken quantity still allows
    half = V // 2
    assert _kind(full, pair, op, s=A + half * ss).vec == half
    assert _kind(full, pair, op, d=A + half * ds).vec == half
    assert _kind(full, pair, op, s=A + ss).vec == 1
    assert _kind(((64, 5), (1, 80), 8 + half, (1, 64), 16), pair, op).vec \
        == half
    assert _kind(((64, 5), (1, 80), 8, (1, 64), 16 + 1), pair, op).vec == 1
    assert _kind(((64, 5), (1, 80 + half), 8, (1, 64), 16), pair, op).vec \
        == half
    assert _kind(((64, 5), (1, 80), 8, (1, 64 + 1), 16), pair, op).vec == 1
    assert _kind(((64 + half, 5), (1, 80), 8, (1, 72), 16), pair, op).vec \
        == half
    assert _kind(((63, 5), (1, 80), 8, (1, 64), 16), pair, op).vec == 1
    # components join the run: 3 scalars x 5 elements is odd, x 4 is not
    assert _kind(((5, 3), (1, 8), 0, (1, 8), 0), pair, op, nc=3).vec == 1
    assert _kind(((4, 3), (1, 8), 0, (1, 8), 0), pair, op, nc=3).vec == V


@pytest.mark.parametrize("pair", list(PAIRS))
def test_selection_tile_generic_none(pair):
    tr = ((40, 50, 3), (1, 40, 2000), 0, (50, 1, 2000), 0)
    for nc in (1, 2, 3, 4):
        for op in (NARROW, WIDEN, ROUND):
            k = _kind(tr, pair, op, nc)
            assert k.kind == native.KERNEL_CVT_TILE and k.vec == 1
            assert k.tile_i > 0 and k.tile_j > 0 and k.sweep_depth == 1
    assert _kind(tr, pair, ROUND, 5) == \
        (native.KERNEL_CVT_GENERIC, 1, 0, 0, 1)
    nocontig = ((7, 5), (2, 20), 0, (3, 40), 0)
    assert _kind(nocontig, pair, NARROW).kind == native.KERNEL_CVT_GENERIC
    empty = ((0, 5), (1, 8), 0, (1, 8), 0)
    assert _kind(empty, pair, NARROW) == (native.KERNEL_NONE, 1, 0, 0, 1)


# ---- errors -------------------------------------------------------------------

def test_errors_go_through_last_error():
    d = ((8,), (1,), 0, (1,), 0)
    with pytest.raises(RuntimeError, match="wire pair"):
        native.copy_kernel_kind_wire(d, 7, NARROW)
    with pytest.raises(RuntimeError, match="wire pair"):
        native.copy_kernel_kind_wire(d, 0, NARROW)
    with pytest.raises(RuntimeError, match="wire op"):
        native.copy_kernel_kind_wire(d, 1, 3)
    with pytest.raises(RuntimeError, match="ncomp"):
        native.copy_kernel_kind_wire(d, 1, NARROW, 0)
    # the launcher refuses the same before touching a device
    with pytest.raises(RuntimeError, match="wire pair"):
        native.device_copy_wire(d, 9, NARROW, 1, A, A)
    with pytest.raises(RuntimeError, match="wire op"):
        native.device_copy_wire(d, 1, -1, 1, A, A)
    with pytest.raises(RuntimeError, match="ncomp"):
        native.device_copy_wire(d, 1, NARROW, 0, A, A)
    topo = Topology((1, 1))
    Pi = Pencil(topo, (4, 5, 6), (1, 2))
    with pytest.raises(RuntimeError, match="wire pair"):
        native.NativePlan(Pi, Pi, 0, 8, wire=4)
    with pytest.raises(RuntimeError, match="ncomp"):
        native.NativePlan(Pi, Pi, 0, 8, ncomp=0, wire=1)
    lib = native.load()
    assert lib.pa_copy_kernel_kind_wire(
        1, (native.I64 * 1)(8), (native.I64 * 1)(1), native.I64(0),
        (native.I64 * 1)(1), native.I64(0), 1, 0, native.I64(1), None, None,
        None) != 0
    assert b"null" in lib.pa_last_error()


def test_python_rejects_unsupported_pairs():
    topo = Topology((1, 1))
    Pi = Pencil(topo, (4, 5, 6), (1, 2))
    Po = Pencil(topo, (4, 5, 6), (0, 2), permute=(1, 2, 0))

    def pair(dtype):
        return (PencilArray.empty(Po, 0, dtype=dtype),
                PencilArray.empty(Pi, 0, dtype=dtype))

    with pytest.raises(ValueError, match="int32"):
        Transposition(*pair(np.int32), wire_dtype="float32")
    with pytest.raises(ValueError, match="float64 -> float16"):
        Transposition(*pair(np.float64), wire_dtype="float16")
    with pytest.raises(ValueError, match="float32 -> float32"):
        Transposition(*pair(np.float32), wire_dtype="float32")
    with pytest.raises(ValueError, match="float32 -> float32"):
        MultiTransposition([pair(np.float32)[0]], [pair(np.float32)[1]],
                           wire_dtype=np.float32)
    with pytest.raises(ValueError, match="unsupported wire dtype"):
        Transposition(*pair(np.float64), wire_dtype="int8")
    with pytest.raises(ValueError):
        round_wire(np.zeros(3, np.int32), "float32")
    t = Transposition(*pair(np.float64))  # None: today's behaviour
    assert t.wire is None


# ---- gloo, world 2 --------------------------------------------------------------

def _gloo_worker(rank, world, port, lib):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        repo = os.path.dirname(here)
        for q in (repo, os.path.join(repo, "oracle"), here):
            sys.path.insert(0, q)
        from pencilarrays_amd import (
            Pencil, PencilArray, Topology, Transposition,
        )
        from wire_util import assert_same, expected_rounded, kind_parents

        cfg = ((16, 21, 41), (2, 1), (1, 2), (0, 1, 2), (0, 2), (1, 2, 0),
               ())
        dims, pdims, di, pi, do, po, extra = cfg
        topo = Topology(pdims)
        Pi = Pencil(topo, dims, di, permute=pi)
        Po = Pencil(topo, dims, do, permute=po)
        parents = kind_parents("f64", dims, pdims, di, extra, 1, lib)
        exp = expected_rounded("f64", parents, cfg, lib)[0]
        src = PencilArray(Pi, rank, parents[0][rank].copy())
        dst = PencilArray.empty(Po, rank)
        Transposition(dst, src, wire_dtype="float32").execute()
        assert_same(dst.data, exp[rank], f"rank {rank}")
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2_wire(oracle_lib_path):
    mp.spawn(_gloo_worker, args=(2, 29843, oracle_lib_path), nprocs=2,
             join=True)
