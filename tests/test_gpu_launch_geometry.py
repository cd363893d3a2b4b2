"""GPU tests of launch geometry at scale: the gridDim.y split of every kernel,
index arithmetic past 2^32 bytes and 2^31 words, the converting fallback past
its block cap, and the eviction of stage tables.

A. Single-descriptor launches whose workgroup count passes the gridDim.x
   limit ``0xFFFFFFFF // threads``: ``bid = blockIdx.y * gridDim.x +
   blockIdx.x`` takes values from a second grid row, and the ``bid >= nblocks``
   guard parks the surplus of the last row.  The tile kernels are selected
   whatever the extents, so ``(2, 2, B)`` with a huge batch ``B`` needs ``B``
   workgroups but only ``4 B`` elements.
B. Grouped launches past the limit: the grid-row boundary falls strictly
   inside the third entry, so ``group_find()`` and the entry-local
   ``bid - first[e]`` run on both sides of it.
C. A small window between a small buffer and a huge one, one side at a time,
   with the window's offset, or its last batch, past 2^32 bytes; for 4-byte
   words and the f32 side of the converting kernels also past word 2^31.
D. ``k_cvt_generic`` with more scalars than ``8192 * 256``: the grid-stride
   loop takes a second trip.
E. More than 12 stage tables on one plan: eviction, rebuild, LRU order, and
   the key change of a staging rebind.

Every case asserts its selection (and for A and B its over-the-limit
workgroup count) on the host before the launch, and compares whole
0xAB-prefilled destinations bit for bit with a reference that is never a
device run of this library: numpy or the C oracle up to about 1.5 GB, plain
torch indexing on the device for the multi-GiB buffers.  Sources are random
bytes, so a workgroup that does the work of the wrong ``bid`` writes other
bytes.  No test holds more than about 9 GiB of device memory.

Left out on purpose:
- ``k_cvt_linear`` past the split needs at least 17 GiB of source;
- the sweep-8 / sweep-32 tile instantiations past the split need more than
  4e9 elements;
- ``k_group_fill`` and ``COPY_1D_NT`` past the split need 64 GiB;
  all of these share the ``bid`` line with kernels that are covered here;
- word index 2^31 in 8- and 16-byte words (the vector-store tile included)
  needs 16 GiB or more; those words are covered past 2^32 bytes only.
"""

import math

import numpy as np
import pytest

from many_util import expected_dests, random_parents
from pencilarrays_amd import (
    MultiTransposition, Pencil, PencilArray, Topology, build_plan,
)

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402
from launch_util import (  # noqa: E402
    DEV, FAR_CVT, FAR_FAMILIES, SENT, assert_split,
    batch_transpose_desc, dev_all, dev_equal, far_window, fill_random,
    first_diff, host_random, host_ref, max_x, run_cvt_past_split, run_far,
    run_past_split,
)
from wire_gpu_util import (  # noqa: E402
    ref_copy, run_copy, side_types, source_values,
)
from wire_gpu_util import transpose_desc as wire_transpose_desc  # noqa: E402
from wire_util import NARROW, PAIRS, ROUND, WIDEN, assert_same  # noqa: E402

KIND = {name: code for code, name in native.KERNEL_NAMES.items()}
ID3 = (0, 1, 2)
GUARD = 256
MX1024, MX512, MX256 = max_x(1024), max_x(512), max_x(256)


# ---- A. single-descriptor launches past the split ------------------------------

# name: (ssz, ncomp, desc, kind, threads per workgroup, workgroups)
SPLIT = {
    "tile_4B": (4, 1, batch_transpose_desc(2, MX1024 + 5), "TILE", 1024,
                4194308),
    "tile_8B_odd_doff": (8, 1, batch_transpose_desc(2, MX1024 + 5, doff=1),
                         "TILE", 1024, 4194308),
    "tile_2B": (2, 1, batch_transpose_desc(2, MX1024 + 5), "TILE", 1024,
                4194308),
    "tile_1B": (1, 1, batch_transpose_desc(3, MX1024 + 5), "TILE", 1024,
                4194308),
    "tile_vs_8B": (8, 1, batch_transpose_desc(2, MX1024 + 5), "TILE_VS",
                   1024, 4194308),
    "tile_16B": (16, 1, batch_transpose_desc(2, MX512 + 5), "TILE", 512,
                 8388612),
    "tile_pk_2B": (2, 1, batch_transpose_desc(4, MX256 + 5), "TILE_PK", 256,
                   16777220),
    "tile_pk_1B": (1, 1, batch_transpose_desc(8, MX256 + 5), "TILE_PK", 256,
                   16777220),
    "tile_wide_3x2B": (2, 3, batch_transpose_desc(2, MX256 + 5), "TILE_WIDE",
                       256, 16777220),
    "tile_wide_5x4B": (4, 5, batch_transpose_desc(2, MX256 + 5), "TILE_WIDE",
                       256, 16777220),
    # two batch axes that cannot merge (padded outer pitches on both sides):
    # the batch decomposition runs on bid values from the second grid row
    "tile_4B_two_batch_axes": (
        4, 1, ((2, 2, 2051, 2047), (1, 2, 5, 5 * 2051 + 3), 3,
               (2, 1, 6, 6 * 2051 + 1), 2), "TILE", 1024, 4198397),
    # the far side of `blocks < max_x` in grid2d(): one workgroup more than
    # gridDim.x can hold
    "tile_4B_limit_plus_1": (4, 1, batch_transpose_desc(2, MX1024 + 1),
                             "TILE", 1024, MX1024 + 1),
}


@pytest.mark.parametrize("case", sorted(SPLIT))
def test_single_launch_past_the_split(case):
    ssz, ncomp, desc, kind, threads, wg = SPLIT[case]
    run_past_split(desc, ssz, ncomp, KIND[kind], threads, 2000 + len(case),
                   want_wg=wg)


def test_single_launch_exactly_at_the_limit():
    """Exactly ``max_x`` workgroups: gridDim.y stays 1 and no workgroup is
    surplus — the near side of ``blocks < max_x`` in grid2d()."""
    run_past_split(batch_transpose_desc(2, MX1024), 4, 1, KIND["TILE"], 1024,
                   2100, want_wg=MX1024, relation="exact")


WIRE_OPS = [NARROW, WIDEN, ROUND]
WIRE_OP_IDS = ["narrow", "widen", "round"]


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("op", WIRE_OPS, ids=WIRE_OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_converting_tile_past_the_split(pair, op, nc):
    """k_cvt_tile, one workgroup per 2 x 2 batch.  The reference converts a
    pool of seeded values on the host and moves random draws from it
    (launch_util.cvt_host_case)."""
    run_cvt_past_split(batch_transpose_desc(2, MX1024 + 5), pair, op, nc,
                       KIND["CVT_TILE"], 1024, 4194308, 2200 + nc)


def test_linear_window_past_the_split():
    """k_copy_linear in byte words: rows of 13 bytes, pitch 15 on the source
    and 17 on the destination, more than 2^32 bytes in all (5 and 5.6 GiB).
    Reference: strided torch views, compared on the device in chunks."""
    rows = (1 << 32) // 13 + 7
    desc = ((13, rows), (1, 15), 0, (1, 17), 0)
    tail = 64
    src = torch.empty(rows * 15, dtype=torch.uint8, device=DEV)
    dst = torch.empty(rows * 17 + tail, dtype=torch.uint8, device=DEV)
    try:
        fill_random(src, 2300)
        dst.fill_(SENT)
        k = native.copy_kernel_kind(desc, 1, src.data_ptr(), dst.data_ptr())
        assert (k.kind, k.word_bytes, k.byteified) == (KIND["LINEAR"], 1, 0)
        wg = math.ceil(13 * rows / 256)
        assert wg > (1 << 24)
        assert_split(wg, 256)
        native.device_copy(desc, 1, src.data_ptr(), dst.data_ptr())
        torch.cuda.synchronize()
        assert dev_equal(dst.as_strided((rows, 13), (17, 1)),
                         src.as_strided((rows, 13), (15, 1)))
        assert dev_all(dst.as_strided((rows, 4), (17, 1), 13), SENT)
        assert dev_all(dst[rows * 17:], SENT)
    finally:
        del src, dst
        torch.cuda.empty_cache()


def test_fill_window_past_the_split():
    """k_fill through pa_device_fill_zero: runs of 13 bytes at pitch 14, more
    than 2^32 bytes to zero (a 4.6 GiB destination); the pad byte of every
    row and the tail keep the sentinel."""
    rows = (1 << 32) // 13 + 7
    desc = ((13, rows), (1, 14), 0)
    tail = 64
    dst = torch.empty(rows * 14 + tail, dtype=torch.uint8, device=DEV)
    try:
        dst.fill_(SENT)
        fk = native.fill_kernel_kind(desc, 1, dst.data_ptr())
        assert (fk.kind, fk.store_bytes) == (KIND["FILL"], 1), fk
        wg = math.ceil(13 * rows / fk.store_bytes / 256)
        assert wg > (1 << 24)
        assert_split(wg, 256)
        native.device_fill_zero(desc, 1, dst.data_ptr())
        torch.cuda.synchronize()
        assert dev_all(dst.as_strided((rows, 13), (14, 1)), 0)
        assert dev_all(dst.as_strided((rows, 1), (14, 1), 13), SENT)
        assert dev_all(dst[rows * 14:], SENT)
    finally:
        del dst
        torch.cuda.empty_cache()


# ---- B. grouped launches past the split ----------------------------------------

def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)


def _assert_straddles(rows, kind, wg, threads):
    """One grouped row of three entries whose workgroups pass the limit, with
    the grid-row boundary strictly inside the third entry."""
    assert [(l.kind, l.grouped, l.entries, l.workgroups) for l in rows] == \
        [(KIND[kind], True, 3, wg)], rows
    assert_split(wg, threads)
    per = wg // 3
    assert 3 * per == wg and 2 * per < max_x(threads) < wg - 1


# (esz, dims, kind, workgroups, threads)
GROUPED_TILE = {
    "4B": (4, (2, 2, 1398103), "TILE", 4194309, 1024),
    "8B": (8, (2, 2, 1398103), "TILE_VS", 4194309, 1024),
    "2B": (2, (2, 2, 1398103), "TILE", 4194309, 1024),
    "16B": (16, (2, 2, 2796205), "TILE", 8388615, 512),
}


@pytest.mark.parametrize("case", list(GROUPED_TILE))
def test_grouped_tile_past_the_split(case, oracle_lib_path):
    """Three fields, x-pencil to y-pencil with permute (1, 0, 2): the batch
    axis cannot merge with the transposed pair, so the stage is one grouped
    tile launch of three entries.  Expectation: the C oracle."""
    esz, dims, kind, wg, threads = GROUPED_TILE[case]
    n = 3
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 0, 2))
    cfg = (dims, (1, 1), (1, 2), ID3, (0, 2), (1, 0, 2), ())
    parents = random_parents(dims, (1, 1), (1, 2), (), esz, n,
                             oracle_lib_path, seed=0x6E0 + esz)
    exp = expected_dests(parents, cfg, esz, oracle_lib_path)
    plan = native.NativePlan(Pi, Po, 0, esz)
    srcs = [_dev(parents[f][0]) for f in range(n)]
    dsts = [_sentinel(len(exp[f][0])) for f in range(n)]
    sp = [t.data_ptr() for t in srcs]
    dp = [t.data_ptr() for t in dsts]
    try:
        _assert_straddles(plan.stage_launches(n, native.STAGE_LOCAL, sp, dp),
                          kind, wg, threads)
        assert plan.stage_launches(n, native.STAGE_PACK, sp, dp) == []
        assert plan.stage_launches(n, native.STAGE_UNPACK, sp, dp) == []
        plan.execute_many(sp, dp, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for f in range(n):
            want = _dev(np.concatenate(
                [exp[f][0], np.full(GUARD, SENT, dtype=np.uint8)]))
            assert torch.equal(dsts[f], want), \
                f"field {f}: " + first_diff(dsts[f], want)
    finally:
        del srcs, dsts, plan
        torch.cuda.empty_cache()


def test_grouped_linear_past_the_split():
    """Three uint8 fields on identity pencils: a grouped k_group_linear in
    byte words (the element count is odd) of 16795461 workgroups against a
    limit of 16777215.  1.43 GB per buffer; compared on the device."""
    dims = (1129, 1153, 1101)
    L = math.prod(dims)
    assert L % 2 == 1
    n = 3
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (1, 2))
    plan = native.NativePlan(Pi, Po, 0, 1)
    srcs = [torch.empty(L, dtype=torch.uint8, device=DEV) for _ in range(n)]
    dsts = [torch.empty(L + GUARD, dtype=torch.uint8, device=DEV)
            for _ in range(n)]
    try:
        for f in range(n):
            fill_random(srcs[f], 2400 + f)
            dsts[f].fill_(SENT)
        sp = [t.data_ptr() for t in srcs]
        dp = [t.data_ptr() for t in dsts]
        _assert_straddles(plan.stage_launches(n, native.STAGE_LOCAL, sp, dp),
                          "LINEAR", 16795461, 256)
        plan.execute_many(sp, dp, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for f in range(n):
            assert dev_equal(dsts[f][:L], srcs[f]), f
            assert dev_all(dsts[f][L:], SENT), f
        # the fields differ, so an entry served from another field's
        # pointers cannot pass
        assert not dev_equal(srcs[0], srcs[1])
    finally:
        del srcs, dsts, plan
        torch.cuda.empty_cache()


# ---- C. far offsets ---------------------------------------------------------------

HUGE_BYTES = (1 << 33) + (1 << 21)


@pytest.fixture(scope="module")
def huge():
    """One 8 GiB (and a little) allocation that every far-offset case takes
    a prefix of as its huge side: as a source it stays uninitialised outside
    the window, as a destination its prefix is refilled with the sentinel."""
    t = torch.empty(HUGE_BYTES, dtype=torch.uint8, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


def _same_bytes(got, exp, what):
    assert got.shape == exp.shape and np.array_equal(got, exp), what


def _far_copy(family, side, how, huge, thresh_bytes):
    ssz, ncomp, kind, shape, sp, dp, odd = FAR_FAMILIES[family]
    B = ssz * ncomp
    win = far_window(shape, sp, dp, odd, side, how, thresh_bytes // B)
    seed = [3000]

    def make_src(n):
        seed[0] += 1
        return host_random(n * B, seed[0])

    def select(desc, s, d):
        k = native.copy_kernel_kind(desc, ssz, s, d, ncomp)
        assert (k.kind, k.byteified) == (KIND[kind], 0), (desc, k)

    run_far(win, B, B, huge, make_src,
            lambda d2, s, d: host_ref(d2, s, d, B), select,
            lambda desc, s, d: native.device_copy(desc, ssz, s, d,
                                                  ncomp=ncomp),
            _same_bytes, thresh_bytes)


@pytest.mark.parametrize("how", ["offset", "batch"])
@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("family", list(FAR_FAMILIES))
def test_window_past_2e32_bytes(family, side, how, huge):
    """The window's offset (``offset``) or its last batch (``batch``) lies
    past byte 2^32 of the huge side; for 1- and 2-byte words that is past
    word 2^31 as well."""
    _far_copy(family, side, how, huge, 1 << 32)


@pytest.mark.parametrize("how", ["offset", "batch"])
@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("family", ["tile_4B", "generic_4B",
                                    "tile_wide_5x4B"])
def test_window_past_word_2e31_in_4_byte_words(family, side, how, huge):
    _far_copy(family, side, how, huge, 1 << 33)


def _far_cvt(family, pair, op, side, how, huge, thresh_bytes):
    nc, kind, shape, sp, dp = FAR_CVT[family]
    st, dt = side_types(pair, op)
    Bs, Bd = st.itemsize * nc, dt.itemsize * nc
    code = PAIRS[pair][2]
    win = far_window(shape, sp, dp, False, side, how,
                     thresh_bytes // (Bs if side == "src" else Bd))
    seed = [3500]

    def make_src(n):
        seed[0] += 1
        return source_values(n * nc, pair, op, seed[0]).view(np.uint8)

    def ref(d2, s, d):
        ref_copy(d2, s.view(st), d.view(dt), nc, pair, op)

    def select(desc, s, d):
        k = native.copy_kernel_kind_wire(desc, code, op, nc, s, d)
        assert k.kind == KIND[kind], (desc, k)

    def same(got, exp, what):
        assert_same(got.view(dt), exp.view(dt), what)

    run_far(win, Bs, Bd, huge, make_src, ref, select,
            lambda desc, s, d: native.device_copy_wire(desc, code, op, nc,
                                                       s, d),
            same, thresh_bytes)


@pytest.mark.parametrize("how", ["offset", "batch"])
@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("op", [NARROW, WIDEN], ids=["narrow", "widen"])
@pytest.mark.parametrize("family", list(FAR_CVT))
def test_converting_window_past_2e32_bytes(family, op, side, how, huge):
    """f32 <-> f16: past byte 2^32 on either side; on the f16 side that is
    past scalar 2^31 too."""
    _far_cvt(family, "f32_f16", op, side, how, huge, 1 << 32)


@pytest.mark.parametrize("how", ["offset", "batch"])
@pytest.mark.parametrize("family", list(FAR_CVT))
def test_converting_window_past_f32_word_2e31(family, how, huge):
    """The f32 side past scalar 2^31 (8 GiB): the source of a narrowing
    copy and the destination of a widening one."""
    _far_cvt(family, "f32_f16", NARROW, "src", how, huge, 1 << 33)
    _far_cvt(family, "f32_f16", WIDEN, "dst", how, huge, 1 << 33)


@pytest.mark.parametrize("how", ["offset", "batch"])
def test_fill_window_past_2e32_bytes(how, huge):
    """pa_device_fill_zero on a (71, 66, 3) byte window far into the huge
    buffer: zeros exactly in the window, the sentinel everywhere else."""
    n0, n1, nb = 71, 66, 3
    pitch = 72
    inner = pitch * n1 + 8
    if how == "offset":
        doff, bstr = (1 << 32) + 8, inner
    else:
        doff, bstr = 8, (1 << 31) + 8
    desc = ((n0, n1, nb), (1, pitch, bstr), doff)
    need = doff + (nb - 1) * bstr + inner + 64
    assert doff + (nb - 1) * bstr > (1 << 32)
    far = huge[:need]
    far.fill_(SENT)
    fk = native.fill_kernel_kind(desc, 1, far.data_ptr())
    assert fk.kind == KIND["FILL"], fk
    native.device_fill_zero(desc, 1, far.data_ptr())
    torch.cuda.synchronize()
    pos = 0
    for b in range(nb):
        lo = doff + b * bstr
        assert dev_all(far[pos:lo], SENT), b
        w = far[lo:lo + pitch * n1].view(n1, pitch)
        assert bool((w[:, :n0] == 0).all()), b
        assert bool((w[:, n0:] == SENT).all()), b
        pos = lo + pitch * n1
    assert dev_all(far[pos:], SENT)


# ---- D. the converting fallback past its block cap ------------------------------

@pytest.mark.parametrize("op", WIRE_OPS, ids=WIRE_OP_IDS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_converting_generic_past_block_cap(pair, op):
    """Five components are past the converting tile; 70 x 66 x 100 elements
    are 2310000 scalars, more than the 8192 x 256 threads of the capped grid,
    so the grid-stride loop of k_cvt_generic takes a second trip."""
    nb = 100
    desc = wire_transpose_desc(70, 66, nb, 75, 3, 69, 2)
    assert 70 * 66 * nb * 5 > 8192 * 256
    run_copy(desc, pair, op, 5, 2500, KIND["CVT_GENERIC"], 1)


# ---- E. stage-table eviction --------------------------------------------------------

TABLES_MAX = 12
E_DIMS = (64, 48, 40)
E_N = 3


def _world1_pencils(dims=E_DIMS):
    topo = Topology((1, 1))
    return (Pencil(topo, dims, (1, 2)),
            Pencil(topo, dims, (0, 2), permute=(1, 2, 0)))


class _ArraySets:
    """Array sets of E_N float64 fields over the world-1 pencil pair, with
    the oracle's destination bytes of each."""

    def __init__(self, oracle_lib_path, seed):
        self.Pi, self.Po = _world1_pencils()
        self.L = self.Pi.length_local(0)
        self.rng = np.random.default_rng(seed)
        self.path = oracle_lib_path
        self.cfg = (E_DIMS, (1, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        self.sets = []

    def add(self):
        src_np = [self.rng.standard_normal(self.L) for _ in range(E_N)]
        exp = [expected_dests([[a.view(np.uint8)]], self.cfg, 8,
                              self.path)[0][0] for a in src_np]
        srcs = [PencilArray(self.Pi, 0, _dev(a)) for a in src_np]
        dsts = [PencilArray(self.Po, 0, torch.full(
            (self.L,), float("nan"), dtype=torch.float64, device=DEV))
            for _ in range(E_N)]
        self.sets.append((srcs, dsts, exp))
        return len(self.sets) - 1

    def point(self, mt, i):
        mt.srcs, mt.dests = self.sets[i][0], self.sets[i][1]

    def clear(self, i):
        for d in self.sets[i][1]:
            d.data.fill_(float("nan"))

    def check(self, i):
        _, dsts, exp = self.sets[i]
        for f in range(E_N):
            got = dsts[f].data.cpu().numpy().view(np.uint8)
            assert got.tobytes() == exp[f].tobytes(), (i, f)

    def ptrs(self, i):
        srcs, dsts, _ = self.sets[i]
        return ([s.data.data_ptr() for s in srcs],
                [d.data.data_ptr() for d in dsts])


def test_eviction_keeps_results_right_and_the_cache_bounded(oracle_lib_path):
    """More array sets than the cache holds tables for, executed back to back
    without a sync in between: every destination of every set equals the
    oracle, the cache never holds more than 12 tables, and a return to the
    first set (evicted by then) rebuilds its tables and is right again."""
    sets = _ArraySets(oracle_lib_path, 31)
    sets.add()
    mt = MultiTransposition(sets.sets[0][1], sets.sets[0][0])
    mt.execute(sync=False)
    nat = mt._native.native
    per_set = nat.stage_table_count()
    assert 1 <= per_set <= 3 and nat.stage_table_builds() == per_set
    nsets = TABLES_MAX // per_set + 2
    for i in range(1, nsets):
        sets.add()
        sets.point(mt, i)
        mt.execute(sync=False)
        assert nat.stage_table_count() == min(TABLES_MAX, (i + 1) * per_set)
        assert nat.stage_table_builds() == (i + 1) * per_set
    mt.wait()
    torch.cuda.synchronize()
    assert nsets * per_set > TABLES_MAX  # tables were evicted
    for i in range(nsets):
        sets.check(i)

    # set 0 holds the oldest tables: all of them are gone by now
    builds = nat.stage_table_builds()
    sets.clear(0)
    sets.point(mt, 0)
    mt.execute()
    torch.cuda.synchronize()
    assert nat.stage_table_builds() == builds + per_set
    assert nat.stage_table_count() == TABLES_MAX
    sets.check(0)


def test_eviction_takes_the_least_recently_used_table(oracle_lib_path):
    """The local stage alone builds one table per array set.  With 12 live
    tables, set 0 is touched and a 13th set comes in: set 1 is now the least
    recently used and must be the one that went.  At capacity a build leaves
    the table count at 12, so the build counter tells a hit from a rebuild;
    torch's allocator sees no allocation in either."""
    sets = _ArraySets(oracle_lib_path, 32)
    plan = native.NativePlan(sets.Pi, sets.Po, 0, 8)
    stream = torch.cuda.current_stream().cuda_stream

    def run(i):
        plan.local_many(*sets.ptrs(i), stream)

    for i in range(TABLES_MAX):
        sets.add()
        run(i)
        assert plan.stage_table_count() == i + 1
    assert plan.stage_table_builds() == TABLES_MAX
    run(0)  # touch: set 1 is the oldest now
    assert plan.stage_table_builds() == TABLES_MAX
    new = sets.add()
    c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    run(new)
    assert plan.stage_table_builds() == TABLES_MAX + 1
    assert plan.stage_table_count() == TABLES_MAX
    run(0)  # still cached
    assert plan.stage_table_builds() == TABLES_MAX + 1, \
        "the touched table was evicted"
    assert plan.stage_table_count() == TABLES_MAX
    for i in range(2, TABLES_MAX):  # as is every set but set 1
        run(i)
    run(new)
    assert plan.stage_table_builds() == TABLES_MAX + 1
    run(1)  # the least recently used set went, and comes back
    assert plan.stage_table_builds() == TABLES_MAX + 2
    assert plan.stage_table_count() == TABLES_MAX
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == c0
    torch.cuda.synchronize()
    for i in range(len(sets.sets)):
        sets.check(i)


def _stage_sim(plans, pyplans, n, sp, dp, sends, recvs):
    """pack -> one slice copy per peer pair -> local -> unpack, all ranks on
    one GPU (the stage simulation of test_gpu_many.py)."""
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
            if sn:
                recvs[blk.global_rank][ro:ro + rn] = sends[r][so:so + sn]
    for r, p in enumerate(plans):
        p.local_many(sp[r], dp[r], stream)
        p.unpack_many(dp[r], stream)
    torch.cuda.synchronize()


def test_staging_rebind_changes_the_table_key(oracle_lib_path):
    """Two simulated ranks whose pack and unpack go through staging.  After
    a set_buffers rebind the tables of the old staging are gone; the old
    staging is then poisoned, so a launch still pointed at it would unpack
    garbage (or pack where the exchange never looks)."""
    dims, pdims = (16, 21, 41), (2,)
    cfg = (dims, pdims, (1,), ID3, (0,), (1, 0, 2), ())
    n, esz, nr = 3, 8, 2
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, (1,))
    Po = Pencil(topo, dims, (0,), permute=(1, 0, 2))
    parents = random_parents(dims, pdims, (1,), (), esz, n, oracle_lib_path,
                             seed=0x7E5)
    exp = expected_dests(parents, cfg, esz, oracle_lib_path)
    pyplans = [build_plan(Pi, Po, r, ()) for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, esz) for r in range(nr)]
    srcs = [[_dev(parents[f][r]) for f in range(n)] for r in range(nr)]
    dsts = [[_sentinel(len(exp[f][r])) for f in range(n)] for r in range(nr)]
    sp = [[t.data_ptr() for t in srcs[r]] for r in range(nr)]
    dp = [[t.data_ptr() for t in dsts[r]] for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    assert all(s > 0 and rb > 0 for s, rb in sizes)  # staging is really used

    def bind():
        sends = [_sentinel(s) for s, _ in sizes]
        recvs = [_sentinel(rb) for _, rb in sizes]
        for r, p in enumerate(plans):
            p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
        return sends, recvs

    def check():
        for r in range(nr):
            for f in range(n):
                nb = len(exp[f][r])
                got = dsts[r][f].cpu().numpy()
                assert got[:nb].tobytes() == exp[f][r].tobytes(), (r, f)
                assert (got[nb:] == SENT).all(), (r, f)

    old = bind()
    _stage_sim(plans, pyplans, n, sp, dp, *old)
    check()
    counts = [p.stage_table_count() for p in plans]
    builds = [p.stage_table_builds() for p in plans]
    assert all(c >= 2 for c in counts)  # pack and unpack at the least

    new = bind()
    assert [p.stage_table_count() for p in plans] == [0] * nr
    for t in old[0] + old[1]:
        t.fill_(0x5C)
    for r in range(nr):
        for d in dsts[r]:
            d.fill_(SENT)
    _stage_sim(plans, pyplans, n, sp, dp, *new)
    check()
    assert [p.stage_table_count() for p in plans] == counts
    assert [p.stage_table_builds() for p in plans] == \
        [b + c for b, c in zip(builds, counts)]
    for sends_or_recvs, col in ((new[0], 0), (new[1], 1)):
        for r, t in enumerate(sends_or_recvs):
            assert bool((t[sizes[r][col]:] == SENT).all()), (r, col)
    for t in old[0] + old[1]:  # nothing wrote the old staging
        assert bool((t == 0x5C).all())
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)
