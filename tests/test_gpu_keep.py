"""Truncated transposes on one MI355X, bit-exact against the C oracle run on
the numpy-masked input.

- pa_device_fill_zero over windows of a small parent, every store width;
- the stage API as a multi-rank run on ONE GPU (the harness of
  test_gpu_many.py): one native keep plan per simulated rank, device slice
  copies at the pa_plan_peer_message ranges standing in for the exchange;
- tile edges of the unpack under truncation, fill boxes next to them;
- Transposition / MultiTransposition with ``keep`` end to end.

Destinations and staging are 0xAB-filled and carry 256-byte guards; whole
buffers are compared as bit patterns, and every case checks the launches it
is about to make through the host queries with the real pointers.
"""

import math

import numpy as np
import pytest

from keep_util import (
    CFG_22, CFG_14, CFG_SLAB, CFG_EMPTY, ID3, check_rows, cfg_id,
    expected_keep, keep_sets,
)
from many_util import random_parents
from pencilarrays_amd import (
    MultiTransposition, Pencil, PencilArray, Topology,
    Transposition, build_plan, fourier_keep,
)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402

GUARD = 256
SENT = 0xAB


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8,
                      device="cuda:0")


def _guard_ok(t, nbytes):
    return bool((t[nbytes:] == SENT).all().item())


# ---- pa_device_fill_zero ----------------------------------------------

PARENT = (67, 35, 5)
PSTR = (1, 67, 67 * 35)


def _box(lo, ext):
    return (tuple(ext), PSTR, sum(l * s for l, s in zip(lo, PSTR)))


FILL_WINDOWS = [
    ("whole", _box((0, 0, 0), PARENT)),
    ("run1", _box((3, 4, 1), (1, 7, 3))),
    ("run15", _box((3, 4, 1), (15, 7, 3))),
    ("run16", _box((4, 4, 1), (16, 7, 3))),
    ("run17", _box((3, 4, 1), (17, 7, 3))),
    ("rows", _box((0, 5, 2), (67, 9, 2))),        # merges into one run
    ("strided0", ((10, 4), (2, 134), 5)),         # not contiguous on axis 0
    ("flat", ((1024,), (1,), 16)),                # 16-byte stores throughout
    ("empty", _box((3, 4, 1), (0, 7, 3))),
]


def _want_store(desc, esz, ptr):
    """The documented width rule, restated: widest of 16/8/4 dividing the
    pointer, the offset, every non-unit stride and the run (or element)."""
    dims, dstr, doff = desc
    if math.prod(dims) == 0:
        return 0
    ax = sorted((s, d) for d, s in zip(dims, dstr) if d != 1) or [(1, 1)]
    merged = [list(ax[0])]
    for s, d in ax[1:]:
        if s == merged[-1][0] * merged[-1][1]:
            merged[-1][1] *= d
        else:
            merged.append([s, d])
    run = merged[0][0] == 1
    unit = merged[0][1] * esz if run else esz
    strides = [s for s, _ in merged[1 if run else 0:]]
    for w in (16, 8, 4):
        if ptr % w == 0 and unit % w == 0 and (doff * esz) % w == 0 and \
                all((s * esz) % w == 0 for s in strides):
            return w
    return 1


@pytest.mark.parametrize("ssz,ncomp", [(1, 1), (2, 1), (4, 1), (8, 1),
                                       (16, 1), (4, 3)],
                         ids=["1B", "2B", "4B", "8B", "16B", "3xf32"])
def test_device_fill_zero(ssz, ncomp):
    esz = ssz * ncomp
    nel = math.prod(PARENT)
    stream = torch.cuda.current_stream().cuda_stream
    widths = set()
    for lead in (0, 1):   # base pointer one element into the allocation
        for name, desc in FILL_WINDOWS:
            if ssz == 16 and lead:
                continue   # a 16-byte scalar needs a 16-byte-aligned base
            nbytes = (nel + lead) * esz
            buf = torch.full((GUARD + nbytes + GUARD,), SENT,
                             dtype=torch.uint8, device="cuda:0")
            base = buf.data_ptr() + GUARD
            assert base % 256 == 0
            ptr = base + lead * esz
            kk = native.fill_kernel_kind(desc, ssz, ptr, ncomp)
            want = _want_store(desc, esz, ptr)
            assert kk == ((native.KERNEL_FILL, want) if want
                          else (native.KERNEL_NONE, 0)), (name, lead)
            widths.add(kk.store_bytes)
            native.device_fill_zero(desc, ssz, ptr, stream, ncomp)
            torch.cuda.synchronize()
            exp = np.full((GUARD + nbytes + GUARD,), SENT, dtype=np.uint8)
            elems = exp[GUARD + lead * esz:GUARD + nbytes].reshape(-1, esz)
            dims, dstr, doff = desc
            if math.prod(dims):
                idx = doff + sum(
                    np.arange(d).reshape([-1 if i == a else 1
                                          for i in range(len(dims))]) * s
                    for a, (d, s) in enumerate(zip(dims, dstr)))
                elems[idx.ravel()] = 0
            assert buf.cpu().numpy().tobytes() == exp.tobytes(), (name, lead)
    assert 0 in widths and 16 in widths
    if esz < 16:                  # the offset base pointer lowers the width
        assert len(widths - {0}) >= 2


# ---- the stage API as a multi-rank run on one GPU ------------------------

def run_stage_sim_keep(cfg, ssz, ncomp, n, keep, fill, oracle_lib_path,
                       parents, aliased=False, on_plan=None):
    """All ranks of ``cfg`` on one GPU through the stage API of keep plans;
    asserts launches, destinations == masked oracle, guards intact."""
    dims, pdims, di, pi, do, po, extra = cfg
    esz = ssz * ncomp
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    zero = fill == native.FILL_ZERO
    exp = expected_keep(parents, cfg, esz, keep, oracle_lib_path,
                        fill_zero=zero, sentinel=SENT)
    pyplans = [build_plan(Pi, Po, r, extra, aliased=aliased, keep=keep,
                          fill=fill) for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, ssz, extra, aliased=aliased,
                               ncomp=ncomp, keep=keep, fill=fill)
             for r in range(nr)]
    srcs = [[_dev(parents[f][r]) if len(parents[f][r]) else _sentinel(0)
             for f in range(n)] for r in range(nr)]
    dsts = [[_sentinel(len(exp[f][r])) for f in range(n)] for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [_sentinel(s) for s, _ in sizes]
    recvs = [_sentinel(rb) for _, rb in sizes]
    sp = [[t.data_ptr() for t in srcs[r]] for r in range(nr)]
    dp = [[t.data_ptr() for t in dsts[r]] for r in range(nr)]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
        local_rows = check_rows(p, pyplans[r], n, ssz, ncomp, sp[r], dp[r],
                                sends[r].data_ptr(), recvs[r].data_ptr())
        if on_plan is not None:
            on_plan(p, pyplans[r], local_rows)

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        p.pack_many(sp[r], stream)
    for r, p in enumerate(plans):
        for blk in pyplans[r].peers:
            if blk.peer_k == pyplans[r].my_k:
                continue
            so, sn, _, _ = p.peer_message(n, blk.peer_k)
            _, _, ro, rn = plans[blk.global_rank].peer_message(
                n, pyplans[r].my_k)
            assert sn == rn
            if sn:   # a zero-byte message is absent from the exchange
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
        # staging is sized in kept bytes; nothing beyond them is written
        assert _guard_ok(sends[r], sizes[r][0]), f"rank {r} send guard"
        assert _guard_ok(recvs[r], sizes[r][1]), f"rank {r} recv guard"
    for p in plans:
        p.set_buffers(0, 0)


STAGE_CFGS = [CFG_22, CFG_14, CFG_SLAB, CFG_EMPTY]
# f64, f32, int16, elem_dims = (3,) of f32
ELEMS = [(8, 1), (4, 1), (2, 1), (4, 3)]
STAGE_KEEPS = ["inside", "droprank", "two_ranges"]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ssz,ncomp", ELEMS,
                         ids=["f64", "f32", "i16", "3xf32"])
@pytest.mark.parametrize("cfg", STAGE_CFGS, ids=cfg_id)
def test_stage_api_multirank_on_one_gpu(cfg, ssz, ncomp, n, oracle_lib_path):
    dims, pdims, di, _, _, _, extra = cfg
    parents = random_parents(dims, pdims, di, extra, ssz * ncomp, n,
                             oracle_lib_path)
    for kname in STAGE_KEEPS:
        for fill in (native.FILL_ZERO, native.FILL_NONE):
            run_stage_sim_keep(cfg, ssz, ncomp, n, keep_sets(cfg)[kname],
                               fill, oracle_lib_path, parents)


@pytest.mark.parametrize("kname", STAGE_KEEPS)
def test_stage_api_aliased_plan(kname, oracle_lib_path):
    """PA_PLAN_ALIASED keep plans: the self block staged per sub-box through
    the recv tail."""
    cfg = CFG_22
    dims, pdims, di, _, _, _, extra = cfg
    parents = random_parents(dims, pdims, di, extra, 8, 3, oracle_lib_path)
    run_stage_sim_keep(cfg, 8, 1, 3, keep_sets(cfg)[kname],
                       native.FILL_ZERO, oracle_lib_path, parents,
                       aliased=True)


# Slab x -> y, permuted output: on rank r the unpack of peer k moves (rank
# r's share of dim 0) x (peer k's share of dim 1) x dim 2, tiled by T_I along
# dim 0 and T_J along dim 1 (128 x 64 for the scalar 8-byte tile).  The keep
# cuts leave sub-boxes of extent T+1 (low range on the first rank), T-1 (high
# range on the last rank) and, with P = 3, 1 (the low range reaching one
# index into the middle rank) along BOTH axes, with fill boxes next to them.
# Entries whose cut keeps the 16-byte alignment run the 64 x 128 vector-store
# tile instead; the same extents are ragged edges of that tile too (127 =
# 2*64 - 1 and 129 = 2*64 + 1 along axis 0, 63 / 65 / 1 inside one tile along
# the other).  Which kernel runs is asserted per entry through the queries.
TI, TJ = 128, 64
EDGE_CFGS = [
    # dims, P, keep dim 0, keep dim 1, extents expected along each axis
    ((260, 132, 3), 2, (TI + 1, TI - 1), (TJ + 1, TJ - 1), (1, -1)),
    ((393, 198, 3), 3, (132, TI - 1), (67, TJ - 1), (0, -1)),
]


@pytest.mark.parametrize("dims,P,k0,k1,rel", EDGE_CFGS,
                         ids=["P2_T+1_T-1", "P3_1_T-1"])
def test_tile_edges_under_truncation(dims, P, k0, k1, rel, oracle_lib_path):
    n = 3
    cfg = (dims, (P,), (1,), ID3, (0,), (1, 0, 2), ())
    keep = [k0, k1, None]
    seen0, seen1, fills = set(), set(), []

    def on_plan(p, pl, local_rows):
        for blk in pl.peers:
            for sb in blk.unpack_subs:
                seen0.add(sb.region[0][1] - sb.region[0][0])
                seen1.add(sb.region[1][1] - sb.region[1][0])
        fills.append(len(pl.fills))
        assert (native.KERNEL_FILL, True, n * len(pl.fills)) in \
            [(l.kind, l.grouped, l.entries) for l in local_rows]

    parents = random_parents(dims, (P,), (1,), (), 8, n, oracle_lib_path)
    run_stage_sim_keep(cfg, 8, 1, n, keep, native.FILL_ZERO, oracle_lib_path,
                       parents, on_plan=on_plan)
    want0 = {1 if rel[0] == 0 else TI + rel[0], TI + rel[1]}
    want1 = {1 if rel[0] == 0 else TJ + rel[0], TJ + rel[1]}
    assert want0 <= seen0, (want0, seen0)
    assert want1 <= seen1, (want1, seen1)
    assert min(fills) >= 1


# ---- end to end, world 1 --------------------------------------------------

W1_DIMS = (130, 67, 35)
W1_KEEP = fourier_keep(W1_DIMS, [43, 22, None], real_dim=0)


def _w1(po):
    topo = Topology((1, 1))
    cfg = (W1_DIMS, (1, 1), (1, 2), ID3, (0, 2), po, ())
    return cfg, Pencil(topo, W1_DIMS, (1, 2)), \
        Pencil(topo, W1_DIMS, (0, 2), permute=po)


def _w1_expected(src_np, cfg, keep, oracle_lib_path):
    return expected_keep([[src_np.view(np.uint8)]], cfg, src_np.itemsize,
                         keep, oracle_lib_path)[0][0]


def _rand(L, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return (rng.standard_normal(L) + 1j * rng.standard_normal(L)
                ).astype(dtype)
    return rng.standard_normal(L).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64],
                         ids=["f64", "c64"])
@pytest.mark.parametrize("po", [ID3, (1, 2, 0)], ids=["identity", "permuted"])
def test_transposition_keep_world1(po, dtype, oracle_lib_path):
    cfg, Pi, Po = _w1(po)
    L = Pi.length_local(0)
    src_np = _rand(L, dtype, 31)
    exp = _w1_expected(src_np, cfg, W1_KEEP, oracle_lib_path)
    src = PencilArray(Pi, 0, _dev(src_np))
    raw = _sentinel(L * src_np.itemsize)
    dst = PencilArray(Po, 0, raw[:L * src_np.itemsize].view(src.data.dtype))
    t = Transposition(dst, src, keep=W1_KEEP)
    t.execute(sync=False)        # deferred wait
    t.wait()
    got = raw.cpu().numpy()
    assert got[:len(exp)].tobytes() == exp.tobytes()
    assert (got[len(exp):] == SENT).all()
    nat = t._native.native
    rows = nat.stage_launches(1, native.STAGE_LOCAL, [src.data.data_ptr()],
                              [dst.data.data_ptr()])
    assert rows[-1].kind == native.KERNEL_FILL and rows[-1].grouped
    assert rows[-1].entries == len(t.plan.fills) > 0
    assert sum(l.entries for l in rows[:-1]) == len(t.plan.local_subs) == 2
    # a repeated call builds and allocates nothing
    tables = nat.stage_table_count()
    assert tables >= 1
    a0 = torch.cuda.memory_allocated()
    raw.fill_(SENT)
    t.execute()
    assert nat.stage_table_count() == tables
    assert torch.cuda.memory_allocated() == a0
    assert raw.cpu().numpy()[:len(exp)].tobytes() == exp.tobytes()
    # fill = None leaves the complement alone
    raw.fill_(SENT)
    Transposition(dst, src, keep=W1_KEEP, fill=None).execute()
    expn = expected_keep([[src_np.view(np.uint8)]], cfg, src_np.itemsize,
                         W1_KEEP, oracle_lib_path, fill_zero=False,
                         sentinel=SENT)[0][0]
    assert raw.cpu().numpy()[:len(expn)].tobytes() == expn.tobytes()


def test_inplace_chain_world1():
    """x -> y -> x in place over one buffer: the masked source."""
    from keep_util import parent_mask
    cfg, Pi, Po = _w1((1, 2, 0))
    L = Pi.length_local(0)
    src_np = _rand(L, np.float64, 32)
    buf = _dev(src_np)
    x, y = PencilArray(Pi, 0, buf), PencilArray(Po, 0, buf)
    fwd = Transposition(y, x, keep=W1_KEEP)
    assert fwd.aliased and fwd.plan.self_pack_subs
    fwd.execute()
    Transposition(x, y, keep=W1_KEEP).execute()
    want = np.where(parent_mask(cfg, W1_KEEP, 0, 0), src_np, 0.0)
    assert buf.cpu().numpy().tobytes() == want.tobytes()


def test_multitransposition_keep_odd_offset_field(oracle_lib_path):
    """Three f64 fields, field 1 living 8 bytes into its allocations: its
    copies and fills lose the 16-byte alignment the others have."""
    cfg, Pi, Po = _w1((1, 2, 0))
    L = Pi.length_local(0)
    src_np = [_rand(L, np.float64, 40 + f) for f in range(3)]
    srcs, dsts, raw = [], [], []
    for f in range(3):
        lead = 1 if f == 1 else 0
        s = torch.empty(L + lead, dtype=torch.float64, device="cuda:0")[lead:]
        s.copy_(torch.from_numpy(src_np[f]))
        d_all = _sentinel((L + lead) * 8).view(torch.uint8)
        raw.append(d_all)
        d = d_all[lead * 8:(lead + L) * 8].view(torch.float64)
        srcs.append(PencilArray(Pi, 0, s))
        dsts.append(PencilArray(Po, 0, d))
    assert dsts[1].data.data_ptr() % 16 == 8
    mt = MultiTransposition(dsts, srcs, keep=W1_KEEP)
    mt.execute()
    nat = mt._native.native
    sp = [s.data.data_ptr() for s in srcs]
    dp = [d.data.data_ptr() for d in dsts]
    check_rows(nat, mt.plan, 3, 8, 1, sp, dp, 0, 0)
    assert native.fill_kernel_kind(mt.plan.fills[0], 8, dp[0]).store_bytes \
        == 16
    assert native.fill_kernel_kind(mt.plan.fills[0], 8, dp[1]).store_bytes \
        == 8
    tables = nat.stage_table_count()
    mt.execute()
    assert nat.stage_table_count() == tables
    for f in range(3):
        lead = 1 if f == 1 else 0
        exp = _w1_expected(src_np[f], cfg, W1_KEEP, oracle_lib_path)
        got = raw[f].cpu().numpy()
        assert got[lead * 8:(lead + L) * 8].tobytes() == exp.tobytes(), f
        assert (got[:lead * 8] == SENT).all()
        assert (got[(lead + L) * 8:] == SENT).all()


def test_execute_fallback_sized_in_kept_bytes(oracle_lib_path):
    """pa_transpose_execute without pa_plan_set_buffers on an aliased keep
    plan: the self block stages through a recv buffer the engine allocates
    itself, sized in kept elements."""
    cfg, Pi, Po = _w1((1, 2, 0))
    L = Pi.length_local(0)
    src_np = _rand(L, np.float64, 33)
    exp = _w1_expected(src_np, cfg, W1_KEEP, oracle_lib_path)
    kept = int(np.prod([a + b for a, b in
                        [(N, 0) if k is None else k
                         for k, N in zip(W1_KEEP, W1_DIMS)]]))
    p = native.NativePlan(Pi, Po, 0, 8, aliased=True, keep=W1_KEEP)
    assert p.buffer_sizes() == (0, kept * 8) and kept < L
    src = _dev(src_np)
    dst = _sentinel(L * 8)
    stream = torch.cuda.current_stream().cuda_stream
    p.execute(src.data_ptr(), dst.data_ptr(), stream)
    p.wait(stream)
    got = dst.cpu().numpy()
    assert got[:L * 8].tobytes() == exp.tobytes()
    assert (got[L * 8:] == SENT).all()


def test_full_keep_is_the_ordinary_transpose():
    cfg, Pi, Po = _w1((1, 2, 0))
    L = Pi.length_local(0)
    src = _dev(_rand(L, np.float64, 34))
    one, two = _sentinel(L * 8), _sentinel(L * 8)
    stream = torch.cuda.current_stream().cuda_stream
    p1 = native.NativePlan(Pi, Po, 0, 8)
    p1.execute(src.data_ptr(), one.data_ptr(), stream)
    keep = [(100, 30), (67, 0), None]      # a + b = N on every dim
    p2 = native.NativePlan(Pi, Po, 0, 8, keep=keep)
    rows = p2.stage_launches(1, native.STAGE_LOCAL, [src.data_ptr()],
                             [two.data_ptr()])
    assert rows and all(l.kind != native.KERNEL_FILL for l in rows)
    p2.execute(src.data_ptr(), two.data_ptr(), stream)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert _guard_ok(two, L * 8)
    assert not (two[:L * 8] == SENT).all().item()
