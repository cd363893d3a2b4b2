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

    def __init__(self):
        self.lines = {q: [] for q in QUERIES}

    def __call__(self, query, key, value):
        self.lines[query].append(f"{key} -> {value!r}")

    def text(self, query):
        return "\n".join(self.lines[query])

    def digest(self):
        h = hashlib.sha256()
        loc = []
        for q in QUERIES:
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


def first_difference(want, got):
    """The first query whose locator differs between two ``[digest,
    locator]`` fixture entries, or None if only the digest does."""
    for i, q in enumerate(QUERIES):
        if want[1][4 * i:4 * i + 4] != got[1][4 * i:4 * i + 4]:
            return q
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", action="store_true",
                    help="write the fixture from the checked-out code")
    ap.add_argument("--dump", metavar="CASE",
                    help="print the full text of one case, for diffing")
    a = ap.parse_args()
    if a.dump:
        c = next(c for c in case_names() if case_id(c) == a.dump)
        rec = record_case(*c)
        for q in QUERIES:
            print(f"== {q}\n{rec.text(q)}")
        return
    cases = {case_id(c): list(record_case(*c).digest()) for c in case_names()}
    if not a.write:
        with open(FIXTURE) as fh:
            want = json.load(fh)["cases"]
        bad = [f"{name}: {first_difference(want[name], got)}"
               for name, got in cases.items() if want.get(name) != got]
        print("\n".join(bad) if bad else f"{len(cases)} cases match")
        sys.exit(1 if bad else 0)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, text=True,
                            capture_output=True).stdout.strip()
    dirty = subprocess.run(
        ["git", "status", "--porcelain", "--", "pencilarrays_amd", "include"],
        cwd=REPO, text=True, capture_output=True).stdout.strip()
    with open(FIXTURE, "w") as fh:
        json.dump({"generated_from_commit": commit + ("+dirty" if dirty else ""),
                   "queries": list(QUERIES), "cases": cases}, fh, indent=0,
                  sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(cases)} cases to {FIXTURE}")


if __name__ == "__main__":
    main()
