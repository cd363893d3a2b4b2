"""Truncated split / join transposes (a keep plan with PA_PLAN_GROUP_SOA) on
one MI355X.

Through ``soa_group_gpu_util.run_hop``: all ranks of a grid on ONE GPU,
results against the C oracle on the numpy-masked (and reference-scaled)
input, staging against the n-field KEEP host run and untouched beyond the
kept bytes, the rows (sub-boxes, then ONE fill row) asserted through the
query with the real pointers before any launch.  Then the classes in world 1
and a grouped tile row past the gridDim.x split."""

import math

import pytest

from keep_util import expected_keep, keep_sets
from soa_group_util import LOCAL, TILE
from soa_scale_util import same, scale_bytes
from soa_util import interleave, split_case

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import max_x  # noqa: E402
from soa_group_gpu_util import (  # noqa: E402
    DEV, GUARD, JOIN, SENT, SPLIT, assert_same_bytes, dev, pencils,
    references, run_hop, sentinel,
)
from test_gpu_soa import STAGE_CFGS  # noqa: E402
from test_gpu_soa_group import _tile_shape  # noqa: E402
from pencilarrays_amd import (  # noqa: E402
    JoinTransposition, Pencil, PencilArray, SplitTransposition, Topology,
    native,
)

ID3 = (0, 1, 2)
DIRS = pytest.mark.parametrize("direction", [SPLIT, JOIN],
                               ids=["split", "join"])
CFGS = [STAGE_CFGS[0], STAGE_CFGS[1], STAGE_CFGS[2], STAGE_CFGS[4]]
NAMES = ["inside", "two_ranges", "two_dims"]
ALPHA = {"f32": -2.0, "f64": 1.0 / 3.0, "c128": 0.5}


@DIRS
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["f32", "f64", "c128"])
@pytest.mark.parametrize("cfg", CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_keep_plans_plain_and_scaled(cfg, kind, n, name, direction,
                                     oracle_lib_path):
    keep = keep_sets(cfg)[name]
    for fill in (native.FILL_ZERO, native.FILL_NONE):
        for alpha in (None, ALPHA[kind]):
            run_hop(cfg, kind, n, direction, oracle_lib_path, keep=keep,
                    fill=fill, alpha=alpha)


@DIRS
@pytest.mark.parametrize("a", [0, 1, 2])
@pytest.mark.parametrize("b", [0, 1, 2])
def test_sub_boxes_at_the_tile_edges_next_to_fill_boxes(a, b, direction,
                                                        oracle_lib_path):
    """A permuted slab over 2 ranks whose shares are e0 + 2 and e1 + 2 wide
    and keep e0 resp. e1 of that at the outer end: every sub-box has extents
    (e0, e1) out of {1, T - 1, T + 1} and a fill box beside it on both
    axes.  f64 x 3."""
    kind, n = "f64", 3
    T = _tile_shape(8, n, direction)
    e0, e1 = [(1, t - 1, t + 1)[i] for t, i in zip(T, (a, b))]
    dims = (2 * (e0 + 2), 2 * (e1 + 2), 3)
    kfull = ((e0, e0), (e1, e1), (3, 0))
    cfg = (dims, (2,), (1,), ID3, (0,), (1, 0, 2), ())
    seen = []

    def check(p, py, aos, fields, send, recv):
        assert p.nfill() > 0
        for which, k in ((0, 0), (2, 0), (2, 1)):
            for s in range(p.nsub(which, k)):
                seen.append(math.prod(p.copydesc_sub(n, 0, which, k, s)[0]))
    run_hop(cfg, kind, n, direction, oracle_lib_path, keep=kfull,
            check=check)
    assert seen == [e0 * e1 * 3] * 4, seen
    run_hop(cfg, kind, n, direction, oracle_lib_path, keep=kfull,
            fill=native.FILL_NONE, alpha=-2.0)


@DIRS
@pytest.mark.parametrize("kind", ["f32", "f64", "c128"])
def test_full_keep_set_equals_the_flagged_ordinary_plan(kind, direction,
                                                        oracle_lib_path):
    cfg, n = STAGE_CFGS[0], 3
    full = tuple((N, 0) for N in cfg[0])
    refs = references(cfg, kind, n, direction, oracle_lib_path)
    ordinary = run_hop(cfg, kind, n, direction, oracle_lib_path, refs=refs)
    kept = run_hop(cfg, kind, n, direction, oracle_lib_path, keep=full)
    assert_same_bytes(ordinary, kept)


# ---- the classes, world 1 ---------------------------------------------------

E2E_DIMS = (130, 67, 35)
E2E_KEEP = ((87, 0), (23, 22), None)
E2E_KFULL = ((87, 0), (23, 22), (35, 0))


def _typed(t, kind):
    return t.view({"f32": torch.float32, "f64": torch.float64,
                   "c128": torch.complex128}[kind])


@pytest.mark.parametrize("fill", ["zero", None])
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "perm"])
def test_classes_world1_with_keep(permuted, fill, oracle_lib_path):
    kind, n, ssz, alpha = "f64", 3, 8, 1.0 / (130 * 67 * 35)
    cfg = (E2E_DIMS, (1, 1), (1, 2), ID3, (0, 2),
           (1, 2, 0) if permuted else ID3, ())
    Pi, Po, _, _ = pencils(cfg)
    aos, comps, _ = split_case(cfg, ssz, n, oracle_lib_path)
    exp = expected_keep(comps, cfg, ssz, E2E_KFULL, oracle_lib_path,
                        fill == "zero", SENT)
    src = PencilArray(Pi, 0, _typed(dev(aos[0]), kind), (), (n,))
    raws = [sentinel(len(exp[c][0])) for c in range(n)]
    dsts = [PencilArray(Po, 0, _typed(raws[c][:len(exp[c][0])], kind))
            for c in range(n)]
    t = SplitTransposition(dsts, src, keep=E2E_KEEP, fill=fill)
    assert t.grouped
    t.execute(sync=False)      # the deferred wait
    t.wait()
    torch.cuda.synchronize()
    assert t._native.native.group_soa()
    for c in range(n):
        got = raws[c].cpu().numpy()
        same(got[:-GUARD], exp[c][0], kind, c)
        assert (got[-GUARD:] == SENT).all()
    # the scaled join of the fields just written, back onto the input pencil
    back_cfg = (E2E_DIMS, (1, 1), (0, 2), cfg[5], (1, 2), ID3, ())
    fields = [[raws[c][:len(exp[c][0])].cpu().numpy().copy()]
              for c in range(n)]
    scaled = [[scale_bytes(x[0], kind, alpha)] for x in fields]
    expj_c = expected_keep(scaled, back_cfg, ssz, E2E_KFULL, oracle_lib_path,
                           fill == "zero", SENT)
    expj = interleave([expj_c[c][0] for c in range(n)], ssz)
    braw = sentinel(len(expj))
    back = PencilArray(Pi, 0, _typed(braw[:len(expj)], kind), (), (n,))
    j = JoinTransposition(back, dsts, scale=alpha, keep=E2E_KEEP, fill=fill)
    j.execute()
    torch.cuda.synchronize()
    got = braw.cpu().numpy()
    same(got[:-GUARD], expj, kind, "join")
    assert (got[-GUARD:] == SENT).all()
    # a repeated call builds and allocates nothing
    builds = [x._native.native.stage_table_builds() for x in (t, j)]
    a0 = torch.cuda.memory_allocated()
    c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    t.execute()
    j.execute()
    assert [x._native.native.stage_table_builds() for x in (t, j)] == builds
    assert torch.cuda.memory_allocated() == a0
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == c0
    same(braw.cpu().numpy()[:-GUARD], expj, kind, "join again")


def test_grouped_false_with_keep_is_refused_before_the_gpu():
    topo = Topology((1, 1))
    Pi = Pencil(topo, (6, 5, 4), (1, 2))
    Po = Pencil(topo, (6, 5, 4), (0, 2))
    a = PencilArray(Pi, 0, torch.zeros(120 * 3, device=DEV,
                                       dtype=torch.float64), (), (3,))
    fs = [PencilArray(Po, 0, torch.zeros(120, device=DEV,
                                         dtype=torch.float64))
          for _ in range(3)]
    with pytest.raises(ValueError, match="grouped=False"):
        SplitTransposition(fs, a, keep=[(4, 0), None, None], grouped=False)
    # grouped=True without keep: the flagged ordinary plan
    t = SplitTransposition(fs, a, grouped=True)
    t.execute()
    assert t._native.native.group_soa()


# ---- launch geometry --------------------------------------------------------

def test_split_tile_row_past_the_grid_split():
    """World 1, (2, 2, Bz) with a permuted output and a keep set of two
    ranges along z: the local stage of the split is ONE grouped SOA_TILE row
    of two (2, 2, B) entries (the sub-boxes of one block are 2^k, so three
    cannot occur on the split side), one workgroup per 2 x 2 batch.  The
    kept planes pass the gridDim.x limit of a 256-wide workgroup and the row
    boundary falls inside the second entry.  f64 x 2, fill none: the three
    dropped planes keep their sentinel.  The reference is torch indexing on
    the device: the buffers are a GiB."""
    n, ssz = 2, 8
    a = max_x(256) // 2
    b = a + 7
    gap = 3
    Bz = a + b + gap
    assert a < max_x(256) < a + b
    dims = (2, 2, Bz)
    topo = Topology((1,))
    Pi = Pencil(topo, dims, (1,))
    Po = Pencil(topo, dims, (0,), permute=(1, 0, 2))
    p = native.NativePlan(Pi, Po, 0, ssz, (), keep=(None, None, (a, b)),
                          fill=native.FILL_NONE, group_soa=True)
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    src = torch.randint(-2 ** 62, 2 ** 62, (4 * Bz * n,), dtype=torch.int64,
                        device=DEV, generator=g)
    f_t = [torch.full((4 * Bz + GUARD // 8,), -1, dtype=torch.int64,
                      device=DEV) for _ in range(n)]
    fp = [t.data_ptr() for t in f_t]
    stg = sentinel(0)
    p.set_buffers(stg.data_ptr(), stg.data_ptr())
    rows = p.stage_launches_soa(n, SPLIT, LOCAL, src.data_ptr(), fp)
    assert [tuple(r) for r in rows] == [(TILE, True, 2, a + b)]
    p.local_split(src.data_ptr(), fp,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s = src.view(Bz, 2, 2, n)                  # z, y, x, c
    for c in range(n):
        o = f_t[c][:4 * Bz].view(Bz, 2, 2)     # z, x, y
        want = s[..., c].permute(0, 2, 1)
        assert torch.equal(o[:a], want[:a]), c
        assert torch.equal(o[Bz - b:], want[Bz - b:]), c
        assert bool((o[a:Bz - b] == -1).all()), c
        assert bool((f_t[c][4 * Bz:] == -1).all()), c
    p.set_buffers(0, 0)
    del src, f_t
    torch.cuda.empty_cache()
