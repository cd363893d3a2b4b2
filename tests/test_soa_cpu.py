"""Split and join transposes, host side (no GPU): the multi-rank simulations
against the C oracle per component, the staging bytes against the n-field
plan on the component copies, the kernel selection through
pa_copy_kernel_kind_soa, and every refusal."""

from __future__ import annotations

import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from soa_util import DTYPES, component, interleave, join_case, split_case
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
from pencilarrays_amd.copyexec import apply_copy
from pencilarrays_amd.plan import build_plan, stage_descs

ID3 = (0, 1, 2)
# (dims, pdims, decomp_in, perm_in, decomp_out, perm_out, extra)
CONFIGS = [
    # the reference chain 1 -> 2 -> 3 with its permutations
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), ()),
    ((16, 21, 41), (2, 2), (0, 2), (1, 2, 0), (0, 1), (2, 1, 0), ()),
    ((16, 21, 41), (1, 4), (1, 2), ID3, (1, 0), (2, 1, 0), ()),
    # without permutations; unsorted decomp dims
    ((16, 21, 41), (2, 2), (1, 2), ID3, (0, 2), ID3, ()),
    ((16, 21, 41), (2, 2), (1, 2), ID3, (1, 0), ID3, ()),
    # the (8,) slab, permuted and not
    ((16, 21, 41), (8,), (1,), ID3, (0,), (1, 0, 2), ()),
    ((16, 21, 41), (8,), (1,), ID3, (0,), ID3, ()),
    # empty ranks: 3 planes over 4 ranks
    ((3, 21, 41), (4, 2), (0, 2), ID3, (1, 2), ID3, ()),
    # 4-D
    ((6, 7, 8, 9), (2, 2), (1, 3), (0, 1, 2, 3), (0, 3), (3, 0, 1, 2), ()),
    # extra dims
    ((8, 9, 10), (2, 2), (1, 2), ID3, (0, 2), (1, 2, 0), (4, 3)),
    # same decomposition: pure local permutation
    ((16, 21, 41), (2, 2), (1, 2), ID3, (1, 2), (2, 0, 1), ()),
]
# (scalar bytes, n, elem_dims)
ELEMS = [(ssz, n, (n,)) for ssz in (4, 8, 16) for n in (2, 3, 4)] + \
    [(ssz, 4, (2, 2)) for ssz in (4, 8, 16)]


def _ids(c):
    return f"{c[0]}x{c[1]}_{c[2]}to{c[4]}_e{c[6]}"


def _eid(e):
    return f"{e[0]}Bx{e[2]}"


def _pencils(cfg):
    dims, pdims, di, pi, do, po, extra = cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po), topo.nranks, extra)


def _arr(P, r, raw, ssz, extra, elem_dims=()):
    return PencilArray(P, r, raw.view(DTYPES[ssz]).copy(), extra, elem_dims)


def _zeros(P, r, nbytes, ssz, extra, elem_dims=()):
    return PencilArray(P, r, np.zeros(nbytes // ssz, dtype=DTYPES[ssz]),
                       extra, elem_dims)


def _many_staging(cfg, ssz, srcs_c, exp_c):
    """Staging of the ordinary n-field plan on scalar sources ``srcs_c[c][r]``
    (bytes), after checking its destinations against ``exp_c``."""
    Pi, Po, nr, extra = _pencils(cfg)
    n = len(srcs_c)
    srcs = [[_arr(Pi, r, srcs_c[c][r], ssz, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp_c[c][r]), ssz, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_many(dsts, srcs, staging_out=staging)
    for r in range(nr):
        for c in range(n):
            assert dsts[r][c].data.tobytes() == exp_c[c][r].tobytes()
    return staging


def _same_staging(a, b):
    for side in ("send", "recv"):
        assert len(a[side]) == len(b[side])
        for x, y in zip(a[side], b[side]):
            assert x.tobytes() == y.tobytes(), side


@pytest.mark.parametrize("ssz,n,elem_dims", ELEMS, ids=lambda v: str(v))
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_split_sim_vs_oracle_and_staging(cfg, ssz, n, elem_dims,
                                         oracle_lib_path):
    Pi, Po, nr, extra = _pencils(cfg)
    aos, comps, exp = split_case(cfg, ssz, n, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], ssz, extra, elem_dims) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), ssz, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging)
    for r in range(nr):
        for c in range(n):
            assert dsts[r][c].data.tobytes() == exp[c][r].tobytes(), (r, c)
        assert srcs[r].data.tobytes() == aos[r].tobytes()  # source untouched
    # every rank's buffers: those of the n-field plan on the component copies
    _same_staging(staging, _many_staging(cfg, ssz, comps, exp))


@pytest.mark.parametrize("ssz,n,elem_dims", ELEMS, ids=lambda v: str(v))
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_join_sim_vs_oracle_and_staging(cfg, ssz, n, elem_dims,
                                        oracle_lib_path):
    Pi, Po, nr, extra = _pencils(cfg)
    fields, exp_c, exp = join_case(cfg, ssz, n, oracle_lib_path)
    srcs = [[_arr(Pi, r, fields[c][r], ssz, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_zeros(Po, r, len(exp[r]), ssz, extra, elem_dims)
            for r in range(nr)]
    staging = {}
    run_transpose_sim_join(dsts, srcs, staging_out=staging)
    for r in range(nr):
        assert dsts[r].data.tobytes() == exp[r].tobytes(), r
    _same_staging(staging, _many_staging(cfg, ssz, fields, exp_c))


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5], CONFIGS[9]], ids=_ids)
def test_split_then_join_round_trip(cfg, oracle_lib_path):
    """x -> y as a split, y -> x as a join: the source comes back."""
    ssz, n = 8, 3
    dims, pdims, di, pi, do, po, extra = cfg
    Pi, Po, nr, _ = _pencils(cfg)
    aos, _, exp = split_case(cfg, ssz, n, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], ssz, extra, (n,)) for r in range(nr)]
    mids = [[_zeros(Po, r, len(exp[c][r]), ssz, extra) for c in range(n)]
            for r in range(nr)]
    run_transpose_sim_split(mids, srcs)
    back = [_zeros(Pi, r, len(aos[r]), ssz, extra, (n,)) for r in range(nr)]
    run_transpose_sim_join(back, mids)
    for r in range(nr):
        assert back[r].data.tobytes() == aos[r].tobytes(), r


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
def test_join_unpack_faces_an_ordinary_pack(cfg, oracle_lib_path):
    """The ordinary n-field pack and exchange fill the buffers; the join runs
    only its local copy and its unpack on them."""
    ssz, n = 8, 3
    Pi, Po, nr, extra = _pencils(cfg)
    fields, exp_c, exp = join_case(cfg, ssz, n, oracle_lib_path)
    staging = _many_staging(cfg, ssz, fields, exp_c)
    srcs = [[_arr(Pi, r, fields[c][r], ssz, extra) for c in range(n)]
            for r in range(nr)]
    dsts = [_zeros(Po, r, len(exp[r]), ssz, extra, (n,)) for r in range(nr)]
    run_transpose_sim_join(dsts, srcs, stages=("local", "unpack"),
                           staging_in=staging)
    for r in range(nr):
        assert dsts[r].data.tobytes() == exp[r].tobytes(), r


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[5]], ids=_ids)
def test_ordinary_unpack_faces_a_split_pack(cfg, oracle_lib_path):
    """The split runs only its pack and the exchange; the local copy and the
    unpack are the ordinary n-field descriptors applied by hand."""
    ssz, n = 8, 3
    Pi, Po, nr, extra = _pencils(cfg)
    aos, comps, exp = split_case(cfg, ssz, n, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], ssz, extra, (n,)) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), ssz, extra) for c in range(n)]
            for r in range(nr)]
    staging = {}
    run_transpose_sim_split(dsts, srcs, staging_out=staging,
                            stages=("pack", "exchange"))
    for r in range(nr):
        plan = build_plan(Pi, Po, r, extra)
        for c in range(n):
            src_c = comps[c][r].view(DTYPES[ssz])
            for _, d in stage_descs(plan, n, c, 1):
                apply_copy(d, src_c, dsts[r][c].data)
            for _, d in stage_descs(plan, n, c, 2):
                apply_copy(d, staging["recv"][r], dsts[r][c].data)
            assert dsts[r][c].data.tobytes() == exp[c][r].tobytes(), (r, c)


def test_sim_rejects_unknown_stage(oracle_lib_path):
    cfg = CONFIGS[0]
    Pi, Po, nr, extra = _pencils(cfg)
    aos, _, exp = split_case(cfg, 8, 2, oracle_lib_path)
    srcs = [_arr(Pi, r, aos[r], 8, extra, (2,)) for r in range(nr)]
    dsts = [[_zeros(Po, r, len(exp[c][r]), 8, extra) for c in range(2)]
            for r in range(nr)]
    with pytest.raises(ValueError, match="unknown stages"):
        run_transpose_sim_split(dsts, srcs, stages=("pack", "send"))


# ---- the classes on numpy arrays ----------------------------------------

@pytest.mark.parametrize("permuted", [False, True])
def test_classes_world1_numpy(permuted, oracle_lib_path):
    ssz, n = 8, 3
    cfg = ((13, 11, 7), (1, 1), (1, 2), ID3, (0, 2),
           (1, 2, 0) if permuted else ID3, ())
    Pi, Po, _, extra = _pencils(cfg)
    aos, _, exp = split_case(cfg, ssz, n, oracle_lib_path)
    src = _arr(Pi, 0, aos[0], ssz, extra, (n,))
    dsts = [_zeros(Po, 0, len(exp[c][0]), ssz, extra) for c in range(n)]
    t = SplitTransposition(dsts, src)
    assert t.execute() is t.dests and t.wait() is t
    for c in range(n):
        assert dsts[c].data.tobytes() == exp[c][0].tobytes()
    back = _zeros(Pi, 0, len(aos[0]), ssz, extra, (n,))
    assert JoinTransposition(back, dsts).execute() is back
    # the reverse hop is the inverse permutation: the source comes back
    assert back.data.tobytes() == aos[0].tobytes()
    again = [_zeros(Po, 0, len(exp[c][0]), ssz, extra) for c in range(n)]
    transpose_split_into(again, src)
    back2 = _zeros(Pi, 0, len(aos[0]), ssz, extra, (n,))
    transpose_join_into(back2, again)
    assert back2.data.tobytes() == aos[0].tobytes()


def _gloo_worker(rank, world, port, lib):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ssz, n = 8, 3
        cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        Pi, Po, _, extra = _pencils(cfg)
        aos, _, exp = split_case(cfg, ssz, n, lib)
        src = _arr(Pi, rank, aos[rank], ssz, extra, (n,))
        dsts = [_zeros(Po, rank, len(exp[c][rank]), ssz, extra)
                for c in range(n)]
        transpose_split_into(dsts, src)
        for c in range(n):
            assert dsts[c].data.tobytes() == exp[c][rank].tobytes(), (rank, c)
        back = _zeros(Pi, rank, len(aos[rank]), ssz, extra, (n,))
        transpose_join_into(back, dsts)
        assert back.data.tobytes() == aos[rank].tobytes(), rank
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2(oracle_lib_path):
    mp.spawn(_gloo_worker, args=(2, 29500 + os.getpid() % 2000,
                                 oracle_lib_path), nprocs=2, join=True)


# ---- Python validation ---------------------------------------------------

def _pair(dtype_a=np.float64, dtype_f=np.float64, n=3, nf=3, elem_dims=None,
          extra_a=(), extra_f=(), field_elem=()):
    topo = Topology((1, 1))
    dims = (6, 5, 4)
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    a = PencilArray.empty(Pi, 0, dtype_a, extra_dims=extra_a,
                          elem_dims=(n,) if elem_dims is None else elem_dims)
    fs = [PencilArray.empty(Po, 0, dtype_f, extra_dims=extra_f,
                            elem_dims=field_elem) for _ in range(nf)]
    return a, fs


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype_f=np.float32), "scalar dtype"),
    (dict(nf=2), "3 scalars per element"),
    (dict(elem_dims=(2, 2)), "4 scalars per element"),
    (dict(elem_dims=()), "scalars per element"),
    (dict(field_elem=(2,)), "cannot have elem_dims"),
    (dict(extra_f=(2,)), "extra dimensions"),
    (dict(nf=1, n=1), "at least 2 fields"),
    (dict(dtype_a=np.float16, dtype_f=np.float16), "4, 8 or 16 bytes"),
], ids=lambda v: str(v) if isinstance(v, str) else "")
def test_python_value_errors(kw, msg):
    a, fs = _pair(**kw)
    with pytest.raises(ValueError, match=msg):
        SplitTransposition(fs, a)
    with pytest.raises(ValueError, match=msg):
        JoinTransposition(a, fs)


def test_python_refuses_aliasing_and_bad_pencils():
    a, fs = _pair()
    with pytest.raises(ValueError, match="must not alias"):
        SplitTransposition([fs[0], fs[1], fs[0]], a)
    flat = np.zeros(len(a.data) + len(fs[0].data))
    a2 = PencilArray(a.pencil, 0, flat[:len(a.data)], (), (3,))
    f2 = PencilArray(fs[0].pencil, 0, flat[2:2 + len(fs[0].data)])
    with pytest.raises(ValueError, match="must not alias"):
        JoinTransposition(a2, [f2, fs[1], fs[2]])
    # a field on another pencil than field 0's
    other = PencilArray.empty(a.pencil, 0)
    with pytest.raises(ValueError, match="pencil differs"):
        SplitTransposition([fs[0], other, fs[2]], a)
    # an incompatible pencil pair: the existing check of the plan builder
    topo = a.pencil.topology
    for Pbad, msg in [
            (Pencil(topo, (6, 5, 5), (0, 2)),
             "global data sizes must be the same"),
            (Pencil(topo, (6, 5, 4), (0, 1)),
             "must differ in at most one dimension")]:
        bad = [PencilArray.empty(Pbad, 0) for _ in range(3)]
        with pytest.raises(ValueError, match=msg):
            SplitTransposition(bad, a)
        with pytest.raises(ValueError, match=msg):
            JoinTransposition(a, bad)


# ---- selection: pa_copy_kernel_kind_soa ----------------------------------

SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN
# a windowed linear copy: runs of 32 scalars, both sides strided
LIN = ((32, 6, 5), (1, 40, 400), 8, (1, 32, 192), 16)


def _kind(desc, ssz, n, d=SPLIT, aos=4096, fields=None):
    return native.copy_kernel_kind_soa(desc, ssz, n, d, aos, fields)


@pytest.mark.parametrize("d", [SPLIT, JOIN])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("ssz", [4, 8, 16])
def test_select_linear_full_v(ssz, n, d):
    k = _kind(LIN, ssz, n, d, fields=[4096 * (c + 2) for c in range(n)])
    assert k == (native.KERNEL_SOA_LINEAR, 16 // ssz, 0, 0, 1)
    # 1-D, and with no field pointers given
    assert _kind(((64,), (1,), 0, (1,), 0), ssz, n, d) == k


def _mod(desc, **kw):
    dims, ss, so, ds, do = [list(x) if isinstance(x, tuple) else x
                            for x in desc]
    out = dict(dims=dims, ss=ss, so=so, ds=ds, do=do)
    for key, (i, v) in kw.items():
        if i is None:
            out[key] = v
        else:
            out[key][i] = v
    return (tuple(out["dims"]), tuple(out["ss"]), out["so"],
            tuple(out["ds"]), out["do"])


@pytest.mark.parametrize("d", [SPLIT, JOIN])
def test_select_linear_v_lowered_one_at_a_time(d):
    ssz, n = 4, 3
    full = [8192, 12288, 16384]

    def v(desc=LIN, aos=4096, fields=full):
        k = _kind(desc, ssz, n, d, aos, fields)
        assert k.kind == native.KERNEL_SOA_LINEAR
        return k.vec

    assert v() == 4
    # the vector-valued array's pointer, then one field pointer
    assert v(aos=4096 + 8) == 2 and v(aos=4096 + 4) == 1
    assert v(fields=[8192, 12288 + 8, 16384]) == 2
    assert v(fields=[8192, 12288, 16384 + 4]) == 1
    # either offset
    assert v(_mod(LIN, so=(None, 10))) == 2
    assert v(_mod(LIN, so=(None, 9))) == 1
    assert v(_mod(LIN, do=(None, 18))) == 2
    assert v(_mod(LIN, do=(None, 17))) == 1
    # a non-unit stride of either side
    assert v(_mod(LIN, ss=(1, 42))) == 2
    assert v(_mod(LIN, ds=(2, 193))) == 1
    # the run length
    assert v(_mod(LIN, dims=(0, 30))) == 2
    assert v(_mod(LIN, dims=(0, 31))) == 1
    # 8-byte scalars: V = 2 down to 1
    k8 = _kind(LIN, 8, n, d, 4096 + 8, full)
    assert (k8.kind, k8.vec) == (native.KERNEL_SOA_LINEAR, 1)


def _wide_shape(B):
    ti = 256
    while ti > 16 and ti * B > 1536:
        ti //= 2
    return ti, 16


# source contiguous along axis 0, destination along axis 2, a batch axis 1
PERM = ((40, 3, 50), (1, 2000, 40), 0, (150, 50, 1), 0)


@pytest.mark.parametrize("d", [SPLIT, JOIN])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("ssz", [4, 8, 16])
def test_select_tile(ssz, n, d):
    k = _kind(PERM, ssz, n, d, 4096 + ssz, [8192 + ssz] * n)
    ti, tj = _wide_shape(ssz * n)
    assert k == (native.KERNEL_SOA_TILE, 1, ti, tj, 1)


@pytest.mark.parametrize("d", [SPLIT, JOIN])
def test_select_generic_and_none(d):
    G = native.KERNEL_SOA_GENERIC
    assert _kind(LIN, 8, 5, d).kind == G          # n = 5
    assert _kind(PERM, 8, 5, d).kind == G
    assert _kind(LIN, 16, 5, d).kind == G         # 16 x 5 bytes
    # no contiguous axis on the destination side, on the source side
    assert _kind(((8, 9), (1, 8), 0, (2, 16), 0), 8, 3, d).kind == G
    assert _kind(((8, 9), (2, 16), 0, (1, 8), 0), 8, 3, d).kind == G
    assert _kind(((8, 9), (3, 24), 0, (9, 1), 0), 8, 3, d).kind == G
    assert _kind(LIN, 8, 5, d) == (G, 1, 0, 0, 1)
    assert _kind(((0, 4), (1, 8), 0, (1, 8), 0), 8, 3, d) == \
        (native.KERNEL_NONE, 1, 0, 0, 1)


@pytest.mark.parametrize("args,msg", [
    ((8, 1, SPLIT), "n must be >= 2"),
    ((8, 0, JOIN), "n must be >= 2"),
    ((2, 3, SPLIT), "invalid scalar_size 2"),
    ((12, 3, SPLIT), "invalid scalar_size 12"),
    ((8, 3, 2), "unknown direction 2"),
])
def test_select_errors(args, msg):
    with pytest.raises(RuntimeError, match=msg):
        _kind(LIN, *args)
    # the copy refuses the same before it touches a pointer
    with pytest.raises(RuntimeError, match=msg):
        native.device_copy_soa(LIN, args[0], max(args[1], 1), args[2], 0,
                               [0] * max(args[1], 1))


@pytest.mark.parametrize("d", [SPLIT, JOIN])
@pytest.mark.parametrize("desc", [LIN, PERM,
                                  ((8, 9), (2, 16), 0, (1, 8), 0)],
                         ids=["linear", "tile", "generic"])
def test_select_refuses_pointers_off_the_scalar(desc, d):
    """A 16-byte scalar moves as one 16-byte word, so 8-byte alignment is not
    enough; nor is 2-byte alignment for a 4-byte one."""
    ok = [8192, 12288, 16384]
    assert _kind(desc, 16, 3, d, 4096, ok).kind != native.KERNEL_NONE
    with pytest.raises(RuntimeError, match="array pointer is not aligned to "
                       "the 16-byte scalar"):
        _kind(desc, 16, 3, d, 4096 + 8, ok)
    with pytest.raises(RuntimeError, match="pointer of field 2 is not "
                       "aligned to the 16-byte scalar"):
        _kind(desc, 16, 3, d, 4096, [8192, 12288, 16384 + 8])
    with pytest.raises(RuntimeError, match="pointer of field 0 is not "
                       "aligned to the 4-byte scalar"):
        _kind(desc, 4, 3, d, 4096, [8192 + 2, 12288, 16384])
    # the copy refuses the same before any launch
    with pytest.raises(RuntimeError, match="not aligned to the 16-byte"):
        native.device_copy_soa(desc, 16, 3, d, 4096 + 8, ok)
    # an empty descriptor touches nothing
    assert _kind(((0, 4), (1, 8), 0, (1, 8), 0), 16, 3, d, 4096 + 8,
                 ok).kind == native.KERNEL_NONE


def test_select_null_output():
    import ctypes
    lib = native.load()
    dims = (native.I64 * 1)(4)
    one = (native.I64 * 1)(1)
    st = lib.pa_copy_kernel_kind_soa(1, dims, one, native.I64(0), one,
                                     native.I64(0), native.I64(8), 3, 0,
                                     ctypes.c_void_p(0), None, None)
    assert st != 0 and b"null output" in lib.pa_last_error()


# ---- the stage calls refuse every other kind of plan ---------------------

def _slab(**kw):
    topo = Topology((2,))
    dims = (8, 6, 4)
    return native.NativePlan(Pencil(topo, dims, (1,)),
                             Pencil(topo, dims, (0,), permute=(1, 0, 2)), 0,
                             kw.pop("esz", 8), (), **kw)


def _all_stage_calls(p, n=3):
    ptrs = [4096 * (c + 2) for c in range(n)]
    return [lambda: p.pack_split(n, 4096),
            lambda: p.local_split(4096, ptrs),
            lambda: p.local_join(ptrs, 4096),
            lambda: p.unpack_join(n, 4096),
            lambda: p.execute_split(4096, ptrs),
            lambda: p.execute_join(ptrs, 4096)]


def _scaled():
    p = _slab()
    p.set_scale(native.SCALAR_F64, 0.5)
    return p


@pytest.mark.parametrize("make,msg", [
    (lambda: _slab(aliased=True),
     "PA_PLAN_ALIASED plan: the two sides have different element sizes"),
    (lambda: _slab(keep=((4, 0), (3, 0), (4, 0))), "keep plan"),
    (lambda: _slab(wire=native.WIRE_F64_F32), "wire plan"),
    (_scaled, "plan with a scale set"),
    (lambda: _slab(ncomp=3), "needs a scalar plan: this one has ncomp = 3"),
    (lambda: _slab(esz=2), "invalid scalar_size 2"),
], ids=["aliased", "keep", "wire", "scale", "composite", "int16"])
def test_stage_calls_refuse_plan_kinds(make, msg):
    p = make()
    for call in _all_stage_calls(p):
        with pytest.raises(RuntimeError, match=msg):
            call()


def test_stage_calls_refuse_bad_arguments():
    p = _slab()
    with pytest.raises(RuntimeError, match="n must be >= 2"):
        p.pack_split(1, 4096)
    with pytest.raises(RuntimeError, match="null vector-valued array"):
        p.pack_split(3, 0)
    with pytest.raises(RuntimeError, match="null pointer for field 1"):
        p.local_split(4096, [8192, 0, 8192])
    # staging must have been set, with the n-field sizes
    with pytest.raises(RuntimeError, match="pa_plan_buffer_sizes_many"):
        p.pack_split(3, 4096)
    with pytest.raises(RuntimeError, match="pa_plan_buffer_sizes_many"):
        p.unpack_join(3, 4096)


def test_component_helpers_are_inverse():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, 5 * 3 * 8, dtype=np.uint8)
    comps = [component(raw, 8, 3, c) for c in range(3)]
    assert comps[1].tobytes() == raw.reshape(5, 3, 8)[:, 1].tobytes()
    assert interleave(comps, 8).tobytes() == raw.tobytes()
