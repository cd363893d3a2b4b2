"""The multi-rank property fuzz of every plan flavour: one configuration
generator, the host references, the selection check and the stage driver.

``draw_cfg(flavour, index)`` draws a trial from a seed derived from
``(flavour, index)`` alone, so a trial is reproducible from its pytest id and
its ``repr`` can be pasted into a named regression test.  ``host_case`` builds
the inputs and the expected destinations of a trial from the per-flavour
references (``many_util``, ``keep_util``, ``wire_util`` / ``wire_group_util``,
``scale_util``, ``soa_util``): the C oracle on the input with the feature
applied in numpy, never a device run.  ``check_selection`` asserts that
``stage_launches`` agrees with the per-descriptor kind queries (host-only: the
pointers are used for their alignment).  ``run_stage_fuzz`` runs every rank of
a trial on one GPU through the stage API and ``run_world1_fuzz`` the Python
classes on one rank; ``compare_dst`` is the comparison both use."""

from __future__ import annotations

import math
import os
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np

import keep_util
import many_util
import scale_util
import soa_util
import wire_gpu_util
import wire_group_util
import wire_util
from pencilarrays_amd import Pencil, Topology, build_plan, native

FLAVOURS = ("plain", "keep", "wire", "wire_group", "scale", "split", "join")
# trials per flavour of the stage-sim tests and of the world-1 group; the
# coverage test pins what these lists reach
DEFAULT_TRIALS = {fl: 24 for fl in FLAVOURS}
WORLD1_TRIALS = 12
SOAK_ENV = "PENCILHIP_FUZZ_MULTIRANK_TRIALS"

# base seed per flavour, chosen on the CPU so that the default lists reach what
# test_fuzz_coverage.py pins
BASE_SEED = {"plain": 5, "keep": 6, "wire": 1, "wire_group": 3, "scale": 2,
             "split": 3, "join": 1}
MAX_ELEMS = 1 << 19    # global elements, extra dims included
MAX_RANKS = 8
GUARD = 256            # guard bytes behind every destination and staging
SENT = 0xAB
A = 4096               # a fake, well aligned address for host-only queries

PLAIN_ELEMS = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (4, 3), (2, 3),
               (4, 5), (8, 2)]
SCALE_ELEMS = ["f32", "f64", "c64", "c128", "3xf32"]
WIRE_ELEMS = [(pair, nc) for nc in (1, 2, 3, 5) for pair in wire_util.PAIRS]
SOA_ELEMS = [4, 8, 16]
ALPHAS = [1.0 / 3.0, -2.5, 2.0 ** -130, 1.0]
CAN_ALIAS = ("plain", "keep", "wire", "wire_group", "scale")
STAGES = (native.STAGE_PACK, native.STAGE_LOCAL, native.STAGE_UNPACK)
SOA_KINDS = {native.KERNEL_SOA_LINEAR, native.KERNEL_SOA_TILE,
             native.KERNEL_SOA_GENERIC}


class Trial(NamedTuple):
    """One drawn configuration.  ``cfg`` = (dims, pdims, di, pi, do, po,
    extra).  ``elem``: (ssz, ncomp) for plain and keep, a ``scale_util.KINDS``
    name for scale, (pair, nc) for the wire flavours, the scalar size for
    split and join.  ``lead`` = (side, j): buffer ``j`` of the "src" or "dst"
    side starts one scalar into its allocation."""
    flavour: str
    index: int
    cfg: tuple
    elem: object
    n: int
    aliased: bool = False
    keep: Optional[tuple] = None
    fill: int = native.FILL_ZERO
    alpha: Optional[float] = None
    lead: Optional[Tuple[str, int]] = None


def trial_count(flavour: str, world1: bool = False) -> int:
    """Trials of a flavour: the committed default, or more with
    ``PENCILHIP_FUZZ_MULTIRANK_TRIALS`` set for a soak."""
    default = WORLD1_TRIALS if world1 else DEFAULT_TRIALS[flavour]
    return max(default, int(os.environ.get(SOAK_ENV, "0")))


def trial_id(t: Trial) -> str:
    return f"{t.flavour}-{t.index}"


def nranks(t: Trial) -> int:
    return math.prod(t.cfg[1])


# ---- the generator ---------------------------------------------------------

def _draw_geometry(rng, world1: bool):
    while True:
        nd = int(rng.integers(2, 6))
        # extents 1..24, a share of them 1..3 so that P > N stays likely
        dims = [int(rng.integers(1, 4)) if rng.random() < 0.15
                else int(rng.integers(1, 25)) for _ in range(nd)]
        if rng.random() < 0.3:   # two or more tiles and a ragged tail
            dims[int(rng.integers(0, nd))] = int(rng.integers(130, 301))
        m = int(rng.integers(1, min(nd, 3)))
        pdims = [1 if world1 else int(rng.integers(1, 5)) for _ in range(m)]
        if rng.random() < 0.3:
            # extents and shares in multiples of 8: the strides and offsets
            # that the vector-store and the packed tile need can occur
            dims = [-(-d // 8) * 8 for d in dims]
            pdims = [4 if p == 3 else p for p in pdims]
        pdims = tuple(pdims)
        axes = list(range(nd))
        di = tuple(int(x) for x in rng.permutation(axes)[:m])
        do = list(di)
        avail = [d for d in axes if d not in di]
        if avail and rng.random() < 0.9:
            do[int(rng.integers(0, m))] = int(rng.permutation(avail)[0])
        pi = tuple(int(x) for x in rng.permutation(nd))
        po = tuple(int(x) for x in rng.permutation(nd))
        extra = (int(rng.integers(2, 4)),) if rng.random() < 0.3 else ()
        if math.prod(pdims) > MAX_RANKS:
            continue
        if math.prod(dims) * math.prod(extra or (1,)) > MAX_ELEMS:
            continue
        return (tuple(dims), pdims, di, pi, tuple(do), po, extra)


def _draw_keep(rng, dims, index: int):
    """(a, b) or None per dim; every 8th trial keeps nothing and every 8th
    everything (a + b = N on every dim)."""
    if index % 8 == 3:
        keep = [None] * len(dims)
        keep[int(rng.integers(0, len(dims)))] = (0, 0)
        return tuple(keep)
    if index % 8 == 6:
        out = []
        for N in dims:
            b = int(rng.integers(0, N + 1))
            out.append(None if rng.random() < 0.5 else (N - b, b))
        return tuple(out)
    out = []
    for N in dims:
        if rng.random() < 0.4:
            out.append(None)
            continue
        lo = N // 2 if rng.random() < 0.7 else 0
        a = int(rng.integers(lo, N + 1))
        b = int(rng.integers(0, N - a + 1)) if rng.random() < 0.4 else 0
        out.append((a, b))
    return tuple(out)


def draw_cfg(flavour: str, index: int, world1: bool = False) -> Trial:
    """Trial ``index`` of ``flavour`` (``world1``: the one-rank group)."""
    rng = np.random.default_rng(
        [BASE_SEED[flavour], FLAVOURS.index(flavour), int(world1), index])
    cfg = _draw_geometry(rng, world1)
    dims = cfg[0]
    n = int(rng.integers(1, 4))
    keep, fill, alpha = None, native.FILL_ZERO, None
    # the element types cycle, so that every one of them comes up
    if flavour in ("plain", "keep"):
        elem = PLAIN_ELEMS[(index + 3 * FLAVOURS.index(flavour))
                           % len(PLAIN_ELEMS)]
    elif flavour == "scale":
        elem = SCALE_ELEMS[index % len(SCALE_ELEMS)]
    elif flavour in ("wire", "wire_group"):
        elem = WIRE_ELEMS[index % len(WIRE_ELEMS)]
    else:
        elem = SOA_ELEMS[index % len(SOA_ELEMS)]
        n = int(rng.integers(2, 5))
    if flavour == "keep" or (flavour == "scale" and rng.random() < 0.5):
        keep = _draw_keep(rng, dims, index)
        fill = native.FILL_ZERO if rng.random() < 0.6 else native.FILL_NONE
    if flavour == "scale":
        alpha = ALPHAS[int(rng.integers(0, len(ALPHAS)))]
    aliased = flavour in CAN_ALIAS and bool(rng.random() < 0.25)
    t = Trial(flavour, index, cfg, elem, n, aliased, keep, fill, alpha)
    lead = None
    if rng.random() < 1.0 / 3.0 and scalar_bytes(t) < 16:
        side = "src" if rng.random() < 0.5 else "dst"
        lead = (side, int(rng.integers(0, n)))
    if world1 and aliased:
        # in place: one buffer holds both sides, so a lead moves both, and
        # what fill = none leaves behind is the source's own bytes
        t = t._replace(fill=native.FILL_ZERO)
    return t._replace(lead=lead)


# ---- what a trial's parameters mean ----------------------------------------

def scalar_bytes(t: Trial) -> int:
    """Bytes of the scalar the trial's plan is created with: pointers must be
    aligned to it, so a lead is one of these."""
    if t.flavour in ("plain", "keep"):
        return t.elem[0]
    if t.flavour == "scale":
        return np.dtype(scale_util.KINDS[t.elem][0]).itemsize
    if t.flavour in ("wire", "wire_group"):
        return np.dtype(wire_util.PAIRS[t.elem[0]][0]).itemsize
    return t.elem


def nbuf(t: Trial, side: str) -> int:
    """Buffers per rank on a side: the vector-valued side of a split or join
    is one array."""
    if (t.flavour, side) in (("split", "src"), ("join", "dst")):
        return 1
    return t.n


def lead_bytes(t: Trial, side: str, j: int, unit: int = 0) -> int:
    """Bytes in front of buffer ``j`` of ``side``: one plan scalar, or
    ``unit`` bytes where an array's item is larger than that."""
    if t.lead is None or t.lead[0] != side:
        return 0
    return (unit or scalar_bytes(t)) if t.lead[1] % nbuf(t, side) == j else 0


def pencils(t: Trial):
    dims, pdims, di, pi, do, po, _ = t.cfg
    topo = Topology(pdims)
    return (Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po))


def has_empty_rank(t: Trial) -> bool:
    """P > N along a decomposed dim: some rank owns nothing on a side."""
    return any(p.length_local(r) == 0 for p in pencils(t)
               for r in range(nranks(t)))


def py_plan(t: Trial, r: int):
    Pi, Po = pencils(t)
    return build_plan(Pi, Po, r, t.cfg[6], aliased=t.aliased, keep=t.keep,
                      fill=t.fill)


def native_plan(t: Trial, r: int, featured: bool = True):
    """The native plan of rank ``r``; ``featured=False`` leaves the scale or
    the grouping flag off (the plan the expected rows are derived from)."""
    Pi, Po = pencils(t)
    extra = t.cfg[6]
    if t.flavour in ("plain", "keep"):
        ssz, ncomp = t.elem
        return native.NativePlan(Pi, Po, r, ssz, extra, aliased=t.aliased,
                                 ncomp=ncomp, keep=t.keep, fill=t.fill)
    if t.flavour in ("wire", "wire_group"):
        pair, nc = t.elem
        return wire_group_util.wire_plan(
            t.cfg, r, pair, nc, t.aliased,
            group_cvt=featured and t.flavour == "wire_group")
    if t.flavour == "scale":
        return scale_util.plan_of(t.cfg, r, t.elem, t.aliased, t.keep, t.fill,
                                  alpha=t.alpha if featured else None)
    return native.NativePlan(Pi, Po, r, t.elem, extra)


# ---- host references --------------------------------------------------------

class Case(NamedTuple):
    """``srcs[r][j]`` / ``exp[r][j]``: source and expected destination
    buffers of rank ``r`` as bytes; ``view``: the scalar type the comparison
    reads them as (None: plain bytes); ``comps[c][r]``: the component copies
    of a split or join source (for the staging reference)."""
    srcs: list
    exp: list
    view: Optional[np.dtype]
    comps: Optional[list] = None


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _by_rank(per_field):
    nr = len(per_field[0])
    return [[_u8(row[r]) for row in per_field] for r in range(nr)]


def host_case(t: Trial, oracle_lib_path: str) -> Case:
    """Inputs (seeded by flavour and index alone) and expected destinations of
    a trial, from the flavour's reference."""
    cfg = t.cfg
    dims, pdims, di, _, _, _, extra = cfg
    seed = zlib.crc32(f"{t.flavour}:{t.index}".encode()) & 0x7FFFFFFF
    zero = t.fill == native.FILL_ZERO
    if t.flavour in ("plain", "keep"):
        esz = t.elem[0] * t.elem[1]
        parents = many_util.random_parents(dims, pdims, di, extra, esz, t.n,
                                           oracle_lib_path, seed)
        if t.flavour == "plain":
            exp = many_util.expected_dests(parents, cfg, esz, oracle_lib_path)
        else:
            exp = keep_util.expected_keep(parents, cfg, esz, t.keep,
                                          oracle_lib_path, fill_zero=zero,
                                          sentinel=SENT)
        return Case(_by_rank(parents), _by_rank(exp), None)
    if t.flavour in ("wire", "wire_group"):
        pair, nc = t.elem
        parents = wire_group_util.parents_of(
            cfg, pair, nc, t.n,
            lambda count, s: wire_util.seeded_values(count, pair, s + seed),
            oracle_lib_path)
        exp = wire_group_util.expected_of(cfg, pair, nc, parents,
                                          oracle_lib_path)
        return Case(_by_rank(parents), _by_rank(exp),
                    np.dtype(wire_util.PAIRS[pair][0]))
    if t.flavour == "scale":
        dtype, _, S, _, nscal = scale_util.KINDS[t.elem]
        parents = scale_util.kind_parents(t.elem, cfg, t.n, oracle_lib_path,
                                          seed)
        if t.keep is None:
            exp = scale_util.expected_scaled(t.elem, parents, cfg, t.alpha,
                                             oracle_lib_path)
        else:
            scaled = [[_u8(scale_util.ref_scale(p, t.alpha)) for p in row]
                      for row in parents]
            exp = keep_util.expected_keep(
                scaled, cfg, np.dtype(S).itemsize * nscal, t.keep,
                oracle_lib_path, fill_zero=zero, sentinel=SENT)
        return Case(_by_rank(parents), _by_rank(exp), np.dtype(S))
    if t.flavour == "split":
        aos, comps, exp_c = soa_util.split_case(cfg, t.elem, t.n,
                                                oracle_lib_path, seed)
        return Case([[_u8(a)] for a in aos], _by_rank(exp_c), None, comps)
    fields, _, exp_aos = soa_util.join_case(cfg, t.elem, t.n, oracle_lib_path,
                                            seed)
    return Case(_by_rank(fields), [[_u8(a)] for a in exp_aos], None, fields)


def as_got(t: Trial, exp):
    """Expected destinations dressed as what the driver reads back: the lead
    and the guard tail around them, sentinel-filled."""
    out = []
    for row in exp:
        bufs = []
        for j, e in enumerate(row):
            lb = lead_bytes(t, "dst", j)
            b = np.full(lb + e.size + GUARD, SENT, dtype=np.uint8)
            b[lb:lb + e.size] = e
            bufs.append(b)
        out.append(bufs)
    return out


def compare_dst(t: Trial, case: Case, got, unit: int = 0) -> None:
    """``got[r][j]``: the WHOLE allocation of destination ``j`` of rank ``r``
    (lead, data, guard) as bytes.  The data bit for bit (as scalars of
    ``case.view``: a NaN for a NaN), lead and guard untouched."""
    for r, row in enumerate(case.exp):
        for j, e in enumerate(row):
            g = got[r][j]
            lb = lead_bytes(t, "dst", j, unit)
            what = f"rank {r} dst {j}: {t!r}"
            assert g.size == lb + e.size + GUARD, what + " size"
            assert (g[:lb] == SENT).all(), what + " lead"
            assert (g[lb + e.size:] == SENT).all(), what + " guard"
            data = g[lb:lb + e.size]
            if case.view is None:
                bad = np.flatnonzero(data != e)
                assert bad.size == 0, \
                    f"{what}: {bad.size} bytes differ, first at {bad[:4]}"
            else:
                wire_util.assert_same(data.view(case.view),
                                      e.view(case.view), what)


# ---- the selection check (host-only) ----------------------------------------

def _ordinary_rows(p, py, t, ssz, ncomp, stages, sp, dp, send, recv):
    n = t.n
    out = []
    for stage in stages:
        got = p.stage_launches(n, stage, sp, dp)
        want = keep_util.expected_rows(py, n, stage, ssz, ncomp, sp, dp, send,
                                       recv)
        assert [(l.kind, l.grouped, l.entries) for l in got] == \
            [(w[0], w[1], w[2]) for w in want], (stage, got, want, t)
        for l, w in zip(got, want):
            if w[3] is not None:
                assert l.workgroups == w[3], (stage, l, w, t)
        out += got
    return out


def _soa_rows(p, py, t, sp, dp, send, recv):
    """The split or join stages have no launch query: the kind query on every
    descriptor they run (it fails on a pointer it cannot take), as
    ungrouped rows; the ordinary n-field stage of the other side as usual."""
    n, ssz = t.n, t.elem
    split = t.flavour == "split"
    direction = native.SOA_SPLIT if split else native.SOA_JOIN
    descs = []   # (descriptor of one component, aos pointer, field pointers)
    if split:
        for b in py.peers:
            if b.pack is not None:
                descs.append((p.copydesc_many(n, 0, 1, b.peer_k), sp[0],
                              [send] * n))
        if py.local is not None:
            descs.append((p.copydesc_many(n, 0, 0), sp[0], dp))
    else:
        if py.local is not None:
            descs.append((p.copydesc_many(n, 0, 0), dp[0], sp))
        for b in py.peers:
            if b.unpack is not None:
                descs.append((p.copydesc_many(n, 0, 2, b.peer_k), dp[0],
                              [recv] * n))
    rows = []
    for d, aos, fields in descs:
        kk = native.copy_kernel_kind_soa(d, ssz, n, direction, aos, fields)
        assert kk.kind in SOA_KINDS | {native.KERNEL_NONE}, (d, kk, t)
        if kk.kind != native.KERNEL_NONE:
            rows.append(native.StageLaunch(kk.kind, False, 1, 0))
    if split:
        rows += _ordinary_rows(p, py, t, ssz, 1, [native.STAGE_UNPACK], None,
                               dp, send, recv)
    else:
        rows += _ordinary_rows(p, py, t, ssz, 1, [native.STAGE_PACK], sp,
                               None, send, recv)
    return rows


def check_selection(t: Trial, r: int, p, py, sp, dp, send=A, recv=A,
                    real: bool = False):
    """Assert that ``stage_launches`` of rank ``r``'s plan ``p`` agrees with
    the per-descriptor kind queries of the flavour, for the source and
    destination pointers ``sp`` / ``dp`` and the staging pointers; returns
    the rows of all stages.  ``real``: the staging pointers are real and set
    on ``p``, so a comparison plan gets them too."""
    n = t.n
    if t.flavour in ("plain", "keep"):
        return _ordinary_rows(p, py, t, t.elem[0], t.elem[1], STAGES, sp, dp,
                              send, recv)
    if t.flavour in ("split", "join"):
        return _soa_rows(p, py, t, sp, dp, send, recv)
    if t.flavour == "wire":
        pair, nc = t.elem
        want = wire_gpu_util._stage_kinds(p, py, n, wire_util.PAIRS[pair][2],
                                          nc, sp, dp, send, recv)
        out = []
        for stage, w in zip(STAGES, want):
            rows = p.stage_launches(n, stage, sp, dp)
            assert [l.kind for l in rows] == w, (r, stage, rows, w, t)
            assert all(l.kind in wire_gpu_util.CVT and not l.grouped
                       for l in rows), (rows, t)
            out += rows
        return out
    plain = native_plan(t, r, featured=False)
    if real:
        plain.set_buffers(send, recv)
    try:
        if t.flavour == "wire_group":
            pair, nc = t.elem
            assert p.group_cvt()
            want = wire_group_util.expected_rows(plain, py, n, pair, nc, sp,
                                                 dp, send, recv)
            got = wire_group_util.flagged_rows(p, n, sp, dp)
        else:
            _, _, _, code, nscal = scale_util.KINDS[t.elem]
            if t.alpha == 1.0:   # takes the scale off: the ordinary rows
                assert p.plan_scale() is None, t
                want = scale_util.plan_rows(plain, n, sp, dp)
            else:
                assert p.plan_scale() == (code, t.alpha), t
                want = scale_util.expected_rows(plain, n, code, nscal, sp, dp,
                                                recv)
            got = scale_util.plan_rows(p, n, sp, dp)
        assert got == want, (r, got, want, t)
    finally:
        if real:
            plain.set_buffers(0, 0)
    return [l for s in STAGES for l in got[s]]


def fake_pointers(t: Trial):
    """Aligned or one-scalar-off addresses, as the drivers lay buffers out."""
    return ([A + lead_bytes(t, "src", j) for j in range(nbuf(t, "src"))],
            [A + lead_bytes(t, "dst", j) for j in range(nbuf(t, "dst"))])


def host_rows(t: Trial):
    """``check_selection`` on every rank with fake pointers; returns
    ``(rows, plans)``: the launch rows of all ranks and the native plans."""
    sp, dp = fake_pointers(t)
    rows, plans = [], []
    for r in range(nranks(t)):
        p = native_plan(t, r)
        rows += check_selection(t, r, p, py_plan(t, r), sp, dp)
        plans.append(p)
    return rows, plans


PLAIN_TILES = {native.KERNEL_TILE, native.KERNEL_TILE_VS,
               native.KERNEL_TILE_PK, native.KERNEL_TILE_WIDE}
FEATURE_TILES = {native.KERNEL_CVT_TILE, native.KERNEL_SCALE_TILE,
                 native.KERNEL_SOA_TILE}


def tile_descriptors(t: Trial):
    """``(dims, ta, tiles)`` of every descriptor of every rank that the
    flavour's kind query gives to an LDS transpose tile, with the fake
    pointers of ``host_rows``: the normalized extents, the
    destination-contiguous axis and the tiles per batch."""
    from pencilarrays_amd.plan import stage_descs
    n = t.n
    sp, dp = fake_pointers(t)
    soa = t.flavour in ("split", "join")
    direction = native.SOA_SPLIT if t.flavour == "split" else native.SOA_JOIN
    out = []

    def add(d, ti, tj):
        ta = next(a for a in range(1, len(d.dims)) if d.dstrides[a] == 1)
        assert d.sstrides[0] == 1, (d, t)
        out.append((d.dims, ta, -(-d.dims[0] // ti) * -(-d.dims[ta] // tj)))

    def plain_query(d, ssz, ncomp, src, dst):
        kk = native.copy_kernel_kind(d, ssz, src, dst, ncomp)
        if kk.kind in PLAIN_TILES:
            tup = keep_util._tup(d)
            one = many_util.expected_workgroups(
                tup, kk._replace(sweep_depth=1), ssz, ncomp)
            ta = next(a for a in range(1, len(d.dims)) if d.dstrides[a] == 1)
            batch = math.prod(d.dims) // (d.dims[0] * d.dims[ta])
            out.append((d.dims, ta, one // batch))

    for r in range(nranks(t)):
        py = py_plan(t, r)
        for f in range(n):
            for stage in STAGES:
                for which, d in stage_descs(py, n, f, stage):
                    if d.nelem == 0:
                        continue
                    if soa:
                        soa_side = which in (0, 1) if t.flavour == "split" \
                            else which in (0, 2)
                        if not soa_side:
                            plain_query(d, t.elem, 1, A, A)
                        elif f == 0:
                            kk = native.copy_kernel_kind_soa(
                                d, t.elem, n, direction, A, [A] * n)
                            if kk.kind in FEATURE_TILES:
                                add(d, kk.tile_i, kk.tile_j)
                        continue
                    src = sp[f] if which in (0, 1, 3) else A
                    dst = A if which in (1, 3) else dp[f]
                    if t.flavour in ("plain", "keep"):
                        plain_query(d, t.elem[0], t.elem[1], src, dst)
                    elif t.flavour == "scale":
                        dtype, elem, _, code, nscal = scale_util.KINDS[t.elem]
                        if which in (1, 3) or t.alpha == 1.0:
                            plain_query(d, np.dtype(dtype).itemsize,
                                        math.prod(elem), src, dst)
                            continue
                        kk = native.copy_kernel_kind_scale(d, code, nscal,
                                                           src, dst)
                        if kk.kind in FEATURE_TILES:
                            add(d, kk.tile_i, kk.tile_j)
                    else:
                        pair, nc = t.elem
                        kk = native.copy_kernel_kind_wire(
                            d, wire_util.PAIRS[pair][2],
                            wire_group_util.WHICH_OP[which], nc, src, dst)
                        if kk.kind in FEATURE_TILES:
                            add(d, kk.tile_i, kk.tile_j)
    return out


# ---- the stage driver: every rank of a trial on one GPU ---------------------

def _host_staging(t: Trial, case: Case):
    """send / recv buffers per rank of the n-field HOST run on the component
    copies of a split or join source."""
    from pencilarrays_amd import PencilArray, run_transpose_sim_many
    Pi, Po = pencils(t)
    extra, ssz, n, nr = t.cfg[6], t.elem, t.n, nranks(t)
    dt = soa_util.DTYPES[ssz]
    srcs = [[PencilArray(Pi, r, case.comps[c][r].view(dt).copy(), extra)
             for c in range(n)] for r in range(nr)]
    dsts = [[PencilArray.empty(Po, r, dtype=dt, extra_dims=extra)
             for c in range(n)] for r in range(nr)]
    out = {}
    run_transpose_sim_many(dsts, srcs, staging_out=out)
    return out


def run_stage_fuzz(t: Trial, oracle_lib_path: str) -> None:
    """One native plan per simulated rank; pack, one device slice copy per
    peer pair at the ``peer_message`` ranges, local, unpack.  Destinations
    and staging are sentinel-filled with a guard tail; the selection is
    asserted with the real pointers before anything launches; whole buffers
    are compared."""
    import torch
    dev = "cuda:0"
    case = host_case(t, oracle_lib_path)
    n, nr = t.n, nranks(t)
    split, join = t.flavour == "split", t.flavour == "join"

    def sentinel(nbytes):
        return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8,
                          device=dev)

    def upload(a, lb):
        body = torch.from_numpy(a).to(dev) if a.size else sentinel(0)
        if not lb:
            return body
        return torch.cat([torch.full((lb,), 0x5C, dtype=torch.uint8,
                                     device=dev), body])

    pyplans = [py_plan(t, r) for r in range(nr)]
    plans = [native_plan(t, r) for r in range(nr)]
    s_all = [[upload(a, lead_bytes(t, "src", j)) for j, a in enumerate(row)]
             for row in case.srcs]
    d_all = [[sentinel(lead_bytes(t, "dst", j) + e.size)
              for j, e in enumerate(row)] for row in case.exp]
    sp = [[x.data_ptr() + lead_bytes(t, "src", j) for j, x in enumerate(row)]
          for row in s_all]
    dp = [[x.data_ptr() + lead_bytes(t, "dst", j) for j, x in enumerate(row)]
          for row in d_all]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [sentinel(s) for s, _ in sizes]
    recvs = [sentinel(rb) for _, rb in sizes]
    try:
        for r, p in enumerate(plans):
            p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
        for r, p in enumerate(plans):
            check_selection(t, r, p, pyplans[r], sp[r], dp[r],
                            sends[r].data_ptr(), recvs[r].data_ptr(),
                            real=True)

        stream = torch.cuda.current_stream().cuda_stream
        for r, p in enumerate(plans):
            if split:
                p.pack_split(n, sp[r][0], stream)
            else:
                p.pack_many(sp[r], stream)
        # the host's exchange: ONE slice copy per peer pair, all fields in it
        for r, p in enumerate(plans):
            for blk in pyplans[r].peers:
                if blk.peer_k == pyplans[r].my_k:
                    continue
                so, sn, _, _ = p.peer_message(n, blk.peer_k)
                _, _, ro, rn = plans[blk.global_rank].peer_message(
                    n, pyplans[r].my_k)
                assert sn == rn, (r, blk.peer_k, sn, rn, t)
                if sn:
                    recvs[blk.global_rank][ro:ro + rn] = sends[r][so:so + sn]
        for r, p in enumerate(plans):
            if split:
                p.local_split(sp[r][0], dp[r], stream)
                p.unpack_many(dp[r], stream)
            elif join:
                p.local_join(sp[r], dp[r][0], stream)
                p.unpack_join(n, dp[r][0], stream)
            else:
                p.local_many(sp[r], dp[r], stream)
                p.unpack_many(dp[r], stream)
        torch.cuda.synchronize()

        compare_dst(t, case, [[x.cpu().numpy() for x in row]
                              for row in d_all])
        ref = _host_staging(t, case) if split or join else None
        for r in range(nr):
            for name, bufs, i in (("send", sends, 0), ("recv", recvs, 1)):
                got, nb = bufs[r].cpu().numpy(), sizes[r][i]
                assert (got[nb:] == SENT).all(), \
                    f"rank {r} {name} guard: {t!r}"
                if ref is not None:
                    assert got[:nb].tobytes() == \
                        _u8(ref[name][r]).tobytes(), \
                        f"rank {r} {name} staging: {t!r}"
        for r, row in enumerate(s_all):   # sources are read-only
            for j, x in enumerate(row):
                lb = lead_bytes(t, "src", j)
                body = x.cpu().numpy()[lb:lb + case.srcs[r][j].size]
                assert body.tobytes() == case.srcs[r][j].tobytes(), \
                    f"rank {r} src {j} changed: {t!r}"
    finally:
        for p in plans:  # tables die with the staging they point into
            p.set_buffers(0, 0)


# ---- world 1: the Python classes end to end on one rank ---------------------

_T_BY_SIZE = {1: "uint8", 2: "int16", 4: "float32", 8: "float64",
              16: "complex128"}


def array_type(t: Trial):
    """``(dtype name, elem_dims)`` (numpy and torch share the names) of the trial's arrays; for a split
    or join, of its scalar fields."""
    if t.flavour in ("plain", "keep"):
        ssz, ncomp = t.elem
        return _T_BY_SIZE[ssz], ((ncomp,) if ncomp > 1 else ())
    if t.flavour == "scale":
        dtype, elem, _, _, _ = scale_util.KINDS[t.elem]
        return np.dtype(dtype).name, tuple(elem)
    if t.flavour in ("wire", "wire_group"):
        pair, nc = t.elem
        stored = np.dtype(wire_util.PAIRS[pair][0])
        if nc == 2:   # a complex item: two stored scalars
            return {4: "complex64", 8: "complex128"}[stored.itemsize], ()
        return stored.name, ((nc,) if nc > 1 else ())
    return _T_BY_SIZE[t.elem], ()


def run_world1_fuzz(t: Trial, oracle_lib_path: str) -> None:
    """A one-rank trial through ``Transposition`` (one field) or
    ``MultiTransposition``, or ``SplitTransposition`` / ``JoinTransposition``,
    on cuda:0; ``aliased`` trials run in place.  A trial that is not in place
    runs twice, the second time from the plan's cached tables."""
    import torch
    from pencilarrays_amd import (
        JoinTransposition, MultiTransposition, PencilArray,
        SplitTransposition, Transposition,
    )
    assert nranks(t) == 1
    dev = "cuda:0"
    case = host_case(t, oracle_lib_path)
    Pi, Po = pencils(t)
    extra, n = t.cfg[6], t.n
    tname, elem_dims = array_type(t)
    tdt = getattr(torch, tname)
    # a lead is one array item: a complex item is two plan scalars
    isz = torch.empty(0, dtype=tdt).element_size()
    inplace = t.aliased
    lead = t.lead if not inplace else (t.lead and ("both", t.lead[1]))

    def lb(side, j):
        if lead is None:
            return 0
        if lead[0] == "both":
            return isz if lead[1] % n == j else 0
        return lead_bytes(t, side, j, isz)

    def typed(raw, off, nbytes):
        return raw[off:off + nbytes].view(tdt)

    def arr(pencil, raw, off, nbytes, ed):
        return PencilArray(pencil, 0, typed(raw, off, nbytes), extra, ed)

    soa = t.flavour in ("split", "join")
    s_ed = (n,) if t.flavour == "split" else elem_dims
    d_ed = (n,) if t.flavour == "join" else elem_dims
    s_raw, d_raw, srcs, dsts = [], [], [], []
    for j, a in enumerate(case.srcs[0]):
        off = lb("src", j)
        nb = max(a.size, case.exp[0][j].size) if inplace else a.size
        raw = torch.full((off + nb + GUARD,), SENT, dtype=torch.uint8,
                         device=dev)
        raw[off:off + a.size] = torch.from_numpy(a).to(dev)
        s_raw.append(raw)
        srcs.append(arr(Pi, raw, off, a.size, s_ed))
    for j, e in enumerate(case.exp[0]):
        off = lb("dst", j)
        raw = s_raw[j] if inplace else torch.full(
            (off + e.size + GUARD,), SENT, dtype=torch.uint8, device=dev)
        d_raw.append(raw)
        dsts.append(arr(Po, raw, off, e.size, d_ed))

    kw = {}
    if t.flavour == "keep" or (t.flavour == "scale" and t.keep is not None):
        kw.update(keep=list(t.keep),
                  fill="zero" if t.fill == native.FILL_ZERO else None)
    if t.flavour == "scale":
        kw.update(scale=t.alpha)
    if t.flavour in ("wire", "wire_group"):
        kw.update(wire_dtype=wire_util.PAIRS[t.elem[0]][1],
                  wire_grouped=t.flavour == "wire_group")
    if t.flavour == "split":
        tr = SplitTransposition(dsts, srcs[0])
    elif t.flavour == "join":
        tr = JoinTransposition(dsts[0], srcs)
    elif n == 1:
        tr = Transposition(dsts[0], srcs[0], **kw)
    else:
        tr = MultiTransposition(dsts, srcs, **kw)
    if not soa:
        assert tr.aliased == inplace, t

    def check(what):
        # whole allocations: lead, data, guard
        got = [x.cpu().numpy() for x in d_raw]
        tt = t._replace(lead=None if lead is None else ("dst", lead[1])) \
            if inplace else t
        try:
            compare_dst(tt, case, [got], isz)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None

    tr.execute(sync=False)
    tr.wait()
    torch.cuda.synchronize()
    check("first run")
    if not inplace:
        builds = tr._native.native.stage_table_builds()
        for j, e in enumerate(case.exp[0]):
            off = lb("dst", j)
            d_raw[j][off:off + e.size] = SENT
        tr.execute()
        torch.cuda.synchronize()
        check("second run")
        assert tr._native.native.stage_table_builds() == builds, \
            f"a repeated call rebuilt a stage table: {t!r}"
