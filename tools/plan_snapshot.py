"""Snapshot of every observable output of the two planners (host-only).

For a fixed matrix of plans this serialises everything ``plan.py`` and the
native planner expose through their public introspection, and reduces it to
one SHA-256 per case plus a 4-hex-digit locator per query, so that a
mismatch can name the first query whose answers changed.  The committed
fixture ``tests/golden/plan_snapshot.json`` pins the planners' behaviour
across refactors of their internal tables; ``tests/test_plan_snapshot.py``
compares against it.

    python tools/plan_snapshot.py --write            # (re)write the fixture
    python tools/plan_snapshot.py --dump CASE        # the full text of a case

The fixture records the commit it was generated from.  It is generated
BEFORE a refactor and committed unchanged with it; regenerating it from the
refactored code would make the comparison empty.

Only public queries are serialised.  On the Python side the ``*_subs``
tables and ``stage_descs`` are public for keep plans only (an ordinary plan
is read through ``pack`` / ``unpack`` / ``local`` / ``self_pack`` /
``self_unpack`` and ``copydesc_many``), so that is where they are recorded.

``--stage`` selects a second matrix with a fixture of its own,
``tests/golden/stage_snapshot.json``: the launch rows of the engine's stage
tables for every plan flavour (see "the stage matrix" below).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from pencilarrays_amd import Pencil, Topology, build_plan, native  # noqa: E402
from pencilarrays_amd import plan as pyplan  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "plan_snapshot.json")

ID3 = (0, 1, 2)
# name: (grid, global size, decomp_in, perm_in, decomp_out, perm_out)
CONFIGS = {
    # 1x1: a one-process subgroup along the differing dim, and R < 0
    "g1x1_d0": ((1, 1), (5, 7, 6), (1, 2), ID3, (0, 2), (1, 2, 0)),
    "g1x1_same": ((1, 1), (5, 7, 6), (1, 2), ID3, (1, 2), (2, 0, 1)),
    # 2x1: each differing dim (P = 2 and P = 1)
    "g2x1_d0": ((2, 1), (5, 7, 6), (1, 2), (1, 2, 0), (0, 2), ID3),
    "g2x1_d1": ((2, 1), (4, 3, 9), (1, 2), (1, 0, 2), (1, 0), (2, 1, 0)),
    # 2x3: each differing dim, uneven blocks, and R < 0
    "g2x3_d0": ((2, 3), (5, 7, 6), (1, 2), ID3, (0, 2), (1, 2, 0)),
    "g2x3_d1": ((2, 3), (4, 3, 9), (0, 1), (2, 0, 1), (0, 2), ID3),
    "g2x3_same": ((2, 3), (4, 3, 9), (0, 2), ID3, (0, 2), (1, 0, 2)),
    # a dim smaller than the subgroup: empty peer blocks and empty ranks
    "g2x3_empty": ((2, 3), (4, 2, 9), (0, 1), ID3, (0, 2), (2, 1, 0)),
}
EXTRAS = ((), (3,), (0,))
WIRE_CONFIG = "g2x3_d0"


def keep_variants(size):
    """name -> (keep, fills): no keep set, a full one (a + b = N merges the
    two ranges), a partial (a, b) one, b = 0, one that empties some peer,
    and one that keeps nothing."""
    n0, n1, n2 = size
    return {
        "none": (None, (1,)),
        "full": ([(n0 - 1, 1), None, (n2, 0)], (1,)),
        "partial": ([(2, 1), None, (2, 2)], (1, 0)),
        "b0": ([(-(-2 * n0 // 3), 0), (-(-2 * n1 // 3), 0),
                (-(-2 * n2 // 3), 0)], (1,)),
        "emptypeer": ([(1, 0), (1, 0), (1, 0)], (1,)),
        "nothing": ([None, (0, 0), None], (1,)),
    }


QUERIES = (
    "py.meta", "py.peers", "py.peer_message", "py.singles",
    "py.copydesc_many", "py.nsub", "py.copydesc_sub", "py.subs", "py.fills",
    "py.stage_descs",
    "nat.meta", "nat.buffer_sizes", "nat.buffer_sizes_many", "nat.block_info",
    "nat.peer_message", "nat.copydesc", "nat.copydesc_many", "nat.nsub",
    "nat.copydesc_sub", "nat.fills", "nat.stage_launches", "nat.kernel_kind",
)
FIELDS = ((1, 0), (3, 0), (3, 2))  # (n, f) pairs queried


def _desc(d):
    if d is None:
        return None
    if hasattr(d, "sstrides"):
        return (d.dims, d.sstrides, d.soffset, d.dstrides, d.doffset)
    return (d.dims, d.dstrides, d.doffset)


def _try(fn):
    try:
        return fn()
    except Exception as e:  # the text of an error is part of the snapshot
        return f"{type(e).__name__}: {e}"


class Recorder:
    """``rec(query, key, value)`` appends one line to the query's stream."""

    def __init__(self, queries=None):
        self.queries = QUERIES if queries is None else queries
        self.lines = {q: [] for q in self.queries}

    def __call__(self, query, key, value):
        self.lines[query].append(f"{key} -> {value!r}")

    def text(self, query):
        return "\n".join(self.lines[query])

    def digest(self):
        h = hashlib.sha256()
        loc = []
        for q in self.queries:
            t = (q + "\n" + self.text(q) + "\n").encode()
            h.update(t)
            loc.append(hashlib.sha256(t).hexdigest()[:4])
        return h.hexdigest(), "".join(loc)


def record_python(rec, tag, pl):
    is_keep = pl.keep is not None
    nk = len(pl.peers)
    ks = list(range(nk)) + [nk]
    rec("py.meta", tag, (
        pl.rank, pl.extra_dims, pl.r_dim, pl.nproc_sub, pl.my_k, pl.aliased,
        pl.keep, pl.fill, pl.send_nelem_total, pl.recv_nelem_total,
        pl.subgroup_global_ranks,
        [pyplan.buffer_nelem_many(pl, n) for n in (1, 3)]))
    for b in pl.peers:
        rec("py.peers", f"{tag} k={b.peer_k}", (
            b.peer_k, b.global_rank, b.send_region, b.recv_region,
            b.send_nelem, b.recv_nelem, b.send_offset, b.recv_offset,
            _desc(b.pack), _desc(b.unpack)))
    for n in (1, 3):
        for k in ks:
            rec("py.peer_message", f"{tag} n={n} k={k}",
                _try(lambda: pyplan.peer_message(pl, n, k)))
    rec("py.singles", tag, (_desc(pl.local), _desc(pl.self_pack),
                            _desc(pl.self_unpack)))
    for which in range(6):
        for k in ks:
            rec("py.nsub", f"{tag} w={which} k={k}",
                _try(lambda: pyplan.nsub(pl, which, k)))
            for n, f in FIELDS:
                rec("py.copydesc_many", f"{tag} n={n} f={f} w={which} k={k}",
                    _try(lambda: _desc(
                        pyplan.copydesc_many(pl, n, f, which, k))))
                ns = pyplan.nsub(pl, which, k) \
                    if is_keep and which < 5 else 0
                for s in range(ns + 1):
                    rec("py.copydesc_sub",
                        f"{tag} n={n} f={f} w={which} k={k} s={s}",
                        _try(lambda: _desc(pyplan.copydesc_sub(
                            pl, n, f, which, k, s))))
    rec("py.fills", tag, [_desc(fd) for fd in pl.fills])
    if is_keep:
        def sub(sb):
            return (sb.region, sb.offset, sb.nelem, _desc(sb.desc))
        rec("py.subs", tag, (
            [[sub(s) for s in b.pack_subs] for b in pl.peers],
            [[sub(s) for s in b.unpack_subs] for b in pl.peers],
            [_desc(d) for d in pl.local_subs],
            [sub(s) for s in pl.self_pack_subs],
            [sub(s) for s in pl.self_unpack_subs]))
        for n, f in FIELDS:
            for stage in range(3):
                rec("py.stage_descs", f"{tag} n={n} f={f} stage={stage}",
                    [(w, _desc(d))
                     for w, d in pyplan.stage_descs(pl, n, f, stage)])


def record_native(rec, tag, nat, ssz, ncomp, wire):
    lib = nat.lib

    def err():
        return "error: " + lib.pa_last_error().decode()

    def opt(v):  # the wrappers answer None where the engine reports an error
        return err() if v is None else v

    npeer = nat.nproc_sub if nat.r_dim >= 0 else 0
    ks = list(range(npeer)) + [npeer]
    rec("nat.meta", tag, (nat.nproc_sub, nat.r_dim, nat.my_k, nat.plan_wire(),
                          nat.plan_keep()))
    rec("nat.buffer_sizes", tag, nat.buffer_sizes())
    for n in (1, 3):
        rec("nat.buffer_sizes_many", f"{tag} n={n}", nat.buffer_sizes_many(n))
    for k in [-1] + ks:
        rec("nat.block_info", f"{tag} k={k}",
            _try(lambda: tuple(int(v) for v in nat.block_info(k))))
        for n in (1, 3):
            rec("nat.peer_message", f"{tag} n={n} k={k}",
                _try(lambda: nat.peer_message(n, k)))
    for which in range(-1, 7):
        for k in ks:
            rec("nat.nsub", f"{tag} w={which} k={k}", nat.nsub(which, k))
            d = nat.copydesc(which, k)
            rec("nat.copydesc", f"{tag} w={which} k={k}", opt(d))
            if d is not None and which < 5:
                rec("nat.kernel_kind", f"{tag} w={which} k={k}",
                    _kind(d, which, ssz, ncomp, wire))
            for n, f in FIELDS:
                rec("nat.copydesc_many", f"{tag} n={n} f={f} w={which} k={k}",
                    opt(nat.copydesc_many(n, f, which, k)))
                ns = nat.nsub(which, k)
                for s in range(ns + 1):
                    d = nat.copydesc_sub(n, f, which, k, s)
                    rec("nat.copydesc_sub",
                        f"{tag} n={n} f={f} w={which} k={k} s={s}", opt(d))
                    if d is not None and n == 1:
                        rec("nat.kernel_kind", f"{tag} w={which} k={k} s={s}",
                            _kind(d, which, ssz, ncomp, wire))
    nf = nat.nfill()
    rec("nat.fills", tag, (nf, [_try(lambda: nat.filldesc(i))
                                for i in range(nf + 1)]))
    for n in (1, 3):
        for stage in range(3):
            rec("nat.stage_launches", f"{tag} n={n} stage={stage}",
                [tuple(r) for r in nat.stage_launches(n, stage)])
    # bad field arguments
    rec("nat.copydesc_many", f"{tag} n=0",
        opt(nat.copydesc_many(0, 0, 0, 0)))
    rec("nat.copydesc_many", f"{tag} n=2 f=2",
        opt(nat.copydesc_many(2, 2, 0, 0)))
    rec("nat.copydesc_sub", f"{tag} n=0",
        opt(nat.copydesc_sub(0, 0, 0, 0, 0)))
    rec("nat.copydesc_sub", f"{tag} n=2 f=2",
        opt(nat.copydesc_sub(2, 2, 0, 0, 0)))


def _kind(d, which, ssz, ncomp, wire):
    if wire is None:
        return tuple(native.copy_kernel_kind(d, ssz, ncomp=ncomp))
    op = (native.WIRE_ROUND if which == 0 else
          native.WIRE_NARROW if which in (1, 3) else native.WIRE_WIDEN)
    return tuple(native.copy_kernel_kind_wire(d, wire, op, ncomp))


def record_case(cfg_name, variant, wire=None):
    """Every query of one case: all ranks, extra dims, aliased on and off,
    the fill modes and the element shapes of the case."""
    grid, size, di, pi, do, po = CONFIGS[cfg_name]
    keep, fills = keep_variants(size)[variant]
    topo = Topology(grid)
    Pi = Pencil(topo, size, di, permute=pi)
    Po = Pencil(topo, size, do, permute=po)
    rec = Recorder()
    for extra in EXTRAS:
        for aliased in (False, True):
            for fill in fills:
                for rank in range(topo.nranks):
                    tag = f"e={extra} al={int(aliased)} fill={fill} r={rank}"
                    if keep is None:
                        pl = build_plan(Pi, Po, rank, extra, aliased=aliased)
                    else:
                        pl = build_plan(Pi, Po, rank, extra, aliased=aliased,
                                        keep=keep, fill=fill)
                    record_python(rec, tag, pl)
                    if wire is not None:
                        shapes = ((4, 1), (4, 2))
                    elif extra == ():
                        shapes = ((8, 1), (4, 3))
                    else:
                        shapes = ((8, 1),)
                    for ssz, ncomp in shapes:
                        nat = native.NativePlan(
                            Pi, Po, rank, ssz, extra, aliased=aliased,
                            ncomp=ncomp, wire=wire, keep=keep, fill=fill)
                        record_native(rec, f"{tag} ssz={ssz} nc={ncomp}", nat,
                                      ssz, ncomp, wire)
    return rec


def case_names():
    out = [(c, v, None) for c in CONFIGS for v in keep_variants((3, 3, 3))]
    out.append((WIRE_CONFIG, "none", native.WIRE_F32_F16))
    return out


def case_id(c):
    cfg, variant, wire = c
    return f"{cfg}/{variant}" + ("/wire" if wire is not None else "")


def first_difference(want, got, queries=QUERIES):
    """The first query whose locator differs between two ``[digest,
    locator]`` fixture entries, or None if only the digest does."""
    for i, q in enumerate(queries):
        if want[1][4 * i:4 * i + 4] != got[1][4 * i:4 * i + 4]:
            return q
    return None


# ---- the stage matrix: launch rows of every plan flavour ------------------
#
# A second fixture, ``tests/golden/stage_snapshot.json``, pins what the
# engine's stage tables decide: the rows of ``pa_plan_stage_launches`` and
# ``pa_plan_stage_launches_soa``, the kernel-kind query of every entry behind
# them, and the error texts, for every plan flavour, on aligned and on offset
# pointers.  ``tests/test_stage_snapshot.py`` compares against it.
#
#     python tools/plan_snapshot.py --stage --write
#     python tools/plan_snapshot.py --stage --dump CASE

STAGE_FIXTURE = os.path.join(REPO, "tests", "golden", "stage_snapshot.json")
STAGE_QUERIES = ("stage.meta", "stage.launches", "stage.kind",
                 "soa.launches", "soa.kind")
STAGE_CONFIGS = tuple(c for c in CONFIGS if c.startswith(("g1x1", "g2x3")))
SOA_NS = (2, 3, 4, 5)

# name: NativePlan arguments, then (scalar, alpha) of pa_plan_set_scale
FLAVOURS = {
    "plain": (dict(elem_size=8), None),
    "comp": (dict(elem_size=4, ncomp=3), None),
    "scale32": (dict(elem_size=4, ncomp=2), (native.SCALAR_F32, 0.5)),
    "scale64": (dict(elem_size=8), (native.SCALAR_F64, 0.25)),
    "keep": (dict(elem_size=8, keep="partial"), None),
    "soa": (dict(elem_size=4), None),
    "soa_group": (dict(elem_size=4, group_soa=True), None),
    "soa_group8": (dict(elem_size=8, group_soa=True), None),
    "keep_soa_group": (dict(elem_size=4, keep="partial", group_soa=True),
                       None),
    # a split or join takes its scale per call; a plan with one set answers
    # the split / join queries with an error text
    "soa_scaled": (dict(elem_size=4, group_soa=True),
                   (native.SCALAR_F32, 0.5)),
}
for _w, _name, _sz in ((native.WIRE_F64_F32, "f64_f32", 8),
                       (native.WIRE_F32_F16, "f32_f16", 4),
                       (native.WIRE_F32_BF16, "f32_bf16", 4)):
    for _nc in (1, 2):
        for _g in (False, True):
            FLAVOURS[f"wire_{_name}_nc{_nc}" + ("_group" if _g else "")] = (
                dict(elem_size=_sz, ncomp=_nc, wire=_w, group_cvt=_g), None)

# Stand-in pointers, never dereferenced.  name: byte offset of pointer i of a
# list; "mixed" offsets field i by 4 * i bytes so the rows of a stage split.
POINTERS = {"a256": lambda i: 0, "o4": lambda i: 4, "o8": lambda i: 8,
            "mixed": lambda i: 4 * (i % 3)}
SRC0, DST0, AOS0, SEND0, RECV0 = (1 << 24, 2 << 24, 3 << 24, 4 << 24, 5 << 24)


def _stage_kind(nat, d, which, scale, src, dst):
    if nat.wire is not None:
        return _kind_ptr(d, which, nat.wire, nat.ncomp, src, dst)
    if scale is not None and which in (0, 2, 4):
        nscal = nat.elem_size * nat.ncomp // native.SCALAR_BYTES[scale[0]]
        return tuple(native.copy_kernel_kind_scale(d, scale[0], nscal, src,
                                                   dst))
    return tuple(native.copy_kernel_kind(d, nat.elem_size, src, dst,
                                         ncomp=nat.ncomp))


def _kind_ptr(d, which, wire, ncomp, src, dst):
    op = (native.WIRE_ROUND if which == 0 else
          native.WIRE_NARROW if which in (1, 3) else native.WIRE_WIDEN)
    return tuple(native.copy_kernel_kind_wire(d, wire, op, ncomp, src, dst))


def _entry_descs(nat, n, f, which, k):
    """The descriptors behind ``which`` of peer ``k`` for field ``f``."""
    if nat.keep is not None:
        return [nat.copydesc_sub(n, f, which, k, s)
                for s in range(nat.nsub(which, k))]
    d = nat.copydesc_many(n, f, which, k)
    return [] if d is None else [d]


def record_stage_plan(rec, tag, nat, scale, off):
    npeer = nat.nproc_sub if nat.r_dim >= 0 else 0
    send, recv = SEND0 + off(0), RECV0 + off(1)
    nat.set_buffers(send, recv)
    rec("stage.meta", tag, (nat.nproc_sub, nat.r_dim, nat.my_k,
                            nat.plan_wire(), nat.plan_keep(),
                            nat.plan_scale(), nat.group_cvt(),
                            nat.group_soa()))
    for n in (1, 3):
        srcs = [SRC0 + (f << 20) + off(f) for f in range(n)]
        dsts = [DST0 + (f << 20) + off(f + 1) for f in range(n)]
        for stage in range(3):
            rec("stage.launches", f"{tag} n={n} stage={stage}",
                _try(lambda: [tuple(r) for r in nat.stage_launches(
                    n, stage, srcs, dsts)]))
        for f in range(n):
            # (which, source, destination) as the stages pair them
            sides = ((0, srcs[f], dsts[f]), (1, srcs[f], send),
                     (2, recv, dsts[f]), (3, srcs[f], recv),
                     (4, recv, dsts[f]))
            for which, src, dst in sides:
                for k in range(npeer if which in (1, 2) else 1):
                    for s, d in enumerate(_entry_descs(nat, n, f, which, k)):
                        rec("stage.kind",
                            f"{tag} n={n} f={f} w={which} k={k} s={s}",
                            _try(lambda: None if d is None else _stage_kind(
                                nat, d, which, scale, src, dst)))
    rec("stage.launches", f"{tag} n=0",
        _try(lambda: nat.stage_launches(0, 0)))
    rec("stage.launches", f"{tag} stage=3",
        _try(lambda: nat.stage_launches(1, 3)))
    for n in SOA_NS:
        aos = AOS0 + off(2)
        fields = [DST0 + (c << 20) + off(c) for c in range(n)]
        for direction in (native.SOA_SPLIT, native.SOA_JOIN):
            for stage in range(3):
                rec("soa.launches", f"{tag} n={n} dir={direction} "
                    f"stage={stage}",
                    _try(lambda: [tuple(r) for r in nat.stage_launches_soa(
                        n, direction, stage, aos, fields)]))
            # local entries with the fields, staged ones on the array alone
            staged = 1 if direction == native.SOA_SPLIT else 2
            for which, fp in ((0, fields), (staged, None)):
                for k in range(npeer if which else 1):
                    for s, d in enumerate(_entry_descs(nat, n, 0, which, k)):
                        rec("soa.kind", f"{tag} n={n} dir={direction} "
                            f"w={which} k={k} s={s}",
                            _try(lambda: None if d is None else tuple(
                                native.copy_kernel_kind_soa(
                                    d, nat.elem_size, n, direction, aos,
                                    fp))))
    rec("soa.launches", f"{tag} n=1",
        _try(lambda: nat.stage_launches_soa(1, native.SOA_SPLIT, 0)))
    rec("soa.launches", f"{tag} dir=7",
        _try(lambda: nat.stage_launches_soa(2, 7, 0)))


def record_stage_case(cfg_name, flavour):
    """Every stage query of one (config, flavour): all ranks, without and
    with an extra dim, on every pointer variant."""
    grid, size, di, pi, do, po = CONFIGS[cfg_name]
    kw, scale = FLAVOURS[flavour]
    kw = dict(kw)
    esz = kw.pop("elem_size")
    if "keep" in kw:
        kw["keep"] = keep_variants(size)[kw["keep"]][0]
    topo = Topology(grid)
    Pi = Pencil(topo, size, di, permute=pi)
    Po = Pencil(topo, size, do, permute=po)
    rec = Recorder(STAGE_QUERIES)
    for extra in ((), (3,)):
        for rank in range(topo.nranks):
            for pname, off in POINTERS.items():
                nat = native.NativePlan(Pi, Po, rank, esz, extra, **kw)
                nat.elem_size = esz
                tag = f"e={extra} r={rank} p={pname}"
                if scale is not None:
                    rec("stage.meta", f"{tag} set_scale",
                        _try(lambda: nat.set_scale(*scale)))
                record_stage_plan(rec, tag, nat, scale, off)
    return rec


def stage_case_names():
    return [(c, f) for c in STAGE_CONFIGS for f in FLAVOURS]


def stage_case_id(c):
    return f"{c[0]}/{c[1]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--stage", action="store_true",
                    help="the stage matrix and its fixture, not the planners'")
    ap.add_argument("--write", action="store_true",
                    help="write the fixture from the checked-out code")
    ap.add_argument("--dump", metavar="CASE",
                    help="print the full text of one case, for diffing")
    a = ap.parse_args()
    if a.stage:
        names, ident, record = stage_case_names(), stage_case_id, \
            record_stage_case
        queries, fixture = STAGE_QUERIES, STAGE_FIXTURE
    else:
        names, ident, record = case_names(), case_id, record_case
        queries, fixture = QUERIES, FIXTURE
    if a.dump:
        c = next(c for c in names if ident(c) == a.dump)
        rec = record(*c)
        for q in queries:
            print(f"== {q}\n{rec.text(q)}")
        return
    cases = {ident(c): list(record(*c).digest()) for c in names}
    if not a.write:
        with open(fixture) as fh:
            want = json.load(fh)["cases"]
        bad = [f"{name}: {first_difference(want[name], got, queries)}"
               for name, got in cases.items() if want.get(name) != got]
        print("\n".join(bad) if bad else f"{len(cases)} cases match")
        sys.exit(1 if bad else 0)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, text=True,
                            capture_output=True).stdout.strip()
    dirty = subprocess.run(
        ["git", "status", "--porcelain", "--", "pencilarrays_amd", "include"],
        cwd=REPO, text=True, capture_output=True).stdout.strip()
    with open(fixture, "w") as fh:
        json.dump({"generated_from_commit": commit + ("+dirty" if dirty else ""),
                   "queries": list(queries), "cases": cases}, fh, indent=0,
                  sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(cases)} cases to {fixture}")


if __name__ == "__main__":
    main()
