"""Stage times of a reduced-precision wire plan against the ordinary plan of
the same pencils, on one GPU.

Slab cases: simulated rank 0 of an (8,) slab, x->y, permuted output pencil;
f64 with the f32 wire at 256^3 and 512^3 for n = 1 and 3 fields, f32 with the
bf16 wire at 512^3 for n = 1.  Per case the pack, local and unpack stage
calls (pa_transpose_{pack,local,unpack}_many) of

  (a) the ordinary plan (code the wire option does not touch: the yardstick),
  (b) the wire plan: NARROW packs, ROUND local copy, WIDEN unpacks, one
      launch per descriptor,
  (c) the wire plan created with PA_PLAN_GROUP_CVT: the same kernels' bodies
      in one grouped launch per stage and signature.

World-1 case: the whole 512^3 permuted x->y transpose (pa_transpose_execute),
ordinary against the two wire plans, each one ROUND copy — what a single-GPU
user pays for the option.

(a), (b) and (c) run in ONE process, alternating a, b, c, a, b, c, ..., each
sample timed with HIP events around the whole stage, after a warm-up of every
shape.  Reported: median of REPS samples with min..max in us, GB/s of the
bytes the stage actually moves (read + written) over the median, and for (c)
against (b) and against (a) whether its median is at or below the other's or
the min..max ranges overlap ("met") or not ("not met").  After the timing the
stages of (b) and (c) run once more on the same inputs and their staging and
destinations are compared byte for byte.  The exchange is not run: one GPU
has nobody to exchange with.

Without --case this is a driver: every case runs as a child process under
its own time limit, one after the other, and the first non-zero status stops
the run.

    python tools/wire_bench.py [--out profiles/wire_bench.txt] [--reps 21]
"""

import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, build_plan, native  # noqa: E402

# name, kind, N, n fields, (stored torch dtype, stored bytes, wire code,
# wire bytes)
F64 = (torch.float64, 8, native.WIRE_F64_F32, 4)
F32 = (torch.float32, 4, native.WIRE_F32_BF16, 2)
CASES = [
    ("slab8 x->y 256^3 f64/f32 n=1", "slab", 256, 1, F64),
    ("slab8 x->y 256^3 f64/f32 n=3", "slab", 256, 3, F64),
    ("slab8 x->y 512^3 f64/f32 n=1", "slab", 512, 1, F64),
    ("slab8 x->y 512^3 f64/f32 n=3", "slab", 512, 3, F64),
    ("slab8 x->y 512^3 f32/bf16 n=1", "slab", 512, 1, F32),
    ("world1 x->y 512^3 f64/f32", "world1", 512, 1, F64),
]
CASE_TIMEOUT_S = 150


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def abc(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    torch.cuda.synchronize()
    return [stats(t) for t in ts]


def met(sc, so):
    """(c) against another leg: met when its median is at or below the
    other's, or the two min..max ranges overlap."""
    (mc, lc, hc), (mo, lo, ho) = sc, so
    return "met" if mc <= mo or not (lc > ho or hc < lo) else "not met"


def line(name, stage, st, nbytes, kinds):
    sa, sb, sc = st
    legs = " | ".join(
        f"{leg} {k} {m:8.1f} ({lo:.1f}..{hi:.1f}) {nb / 1e3 / m:6.0f} GB/s"
        for leg, k, (m, lo, hi), nb in zip(
            ("(a) ordinary", "(b) wire", "(c) wire grouped"), kinds, st,
            nbytes))
    return (f"{name} {stage:6s} {legs} | b/a {sb[0] / sa[0]:.3f} c/a "
            f"{sc[0] / sa[0]:.3f} c/b {sc[0] / sb[0]:.3f} | c<=b "
            f"{met(sc, sb)} | c<=a {met(sc, sa)}")


def kinds_of(rows):
    """The launches of a stage: ``LINEAR[g7]`` = one grouped launch over 7
    descriptors, ``7xCVT_TILE`` = seven launches of that kernel."""
    names = [f"{native.KERNEL_NAMES[r.kind]}"
             f"{'[g' + str(r.entries) + ']' if r.grouped else ''}"
             for r in rows]
    out = []
    for nm in names:
        if out and out[-1][0] == nm:
            out[-1][1] += 1
        else:
            out.append([nm, 1])
    return "+".join(nm if c == 1 else f"{c}x{nm}" for nm, c in out)


def run_slab(name, N, n, elem, reps, warmup, out):
    tdt, ssz, code, wsz = elem
    dims = (N,) * 3
    topo = Topology((8,))
    Pi = Pencil(topo, dims, (1,))
    Po = Pencil(topo, dims, (0,), permute=(1, 0, 2))
    pyp = build_plan(Pi, Po, 0)
    pa = native.NativePlan(Pi, Po, 0, ssz)
    pb = native.NativePlan(Pi, Po, 0, ssz, wire=code)
    pc = native.NativePlan(Pi, Po, 0, ssz, wire=code, group_cvt=True)
    plans = (pa, pb, pc)
    srcs = [torch.randn(Pi.length_local(0), dtype=tdt, device="cuda:0")
            for _ in range(n)]
    dsts = [torch.zeros(Po.length_local(0), dtype=tdt, device="cuda:0")
            for _ in range(n)]
    bufs = []
    for p in plans:
        sb, rb = p.buffer_sizes_many(n)
        send = torch.zeros(sb, dtype=torch.uint8, device="cuda:0")
        # finite wire values to widen: zeros would do, ones show in a diff
        recv = torch.ones(rb, dtype=torch.uint8, device="cuda:0")
        p.set_buffers(send.data_ptr(), recv.data_ptr())
        bufs.append((send, recv))
    sp = [t.data_ptr() for t in srcs]
    dp = [t.data_ptr() for t in dsts]
    n_pack = n * sum(b.send_nelem for b in pyp.peers if b.pack is not None)
    n_unpack = n * sum(b.recv_nelem for b in pyp.peers
                       if b.unpack is not None)
    n_local = n * (pyp.local.nelem if pyp.local is not None else 0)
    stages = [
        ("pack", native.STAGE_PACK, lambda p: (lambda: p.pack_many(sp)),
         n_pack * 2 * ssz, n_pack * (ssz + wsz)),
        ("local", native.STAGE_LOCAL,
         lambda p: (lambda: p.local_many(sp, dp)),
         n_local * 2 * ssz, n_local * 2 * ssz),
        ("unpack", native.STAGE_UNPACK, lambda p: (lambda: p.unpack_many(dp)),
         n_unpack * 2 * ssz, n_unpack * (ssz + wsz)),
    ]
    for sname, stage, mk, bytes_a, bytes_b in stages:
        out(line(name, sname, abc([mk(p) for p in plans], reps, warmup),
                 (bytes_a, bytes_b, bytes_b),
                 [kinds_of(p.stage_launches(n, stage, sp, dp))
                  for p in plans]))
    # (c) computes what (b) computes: every stage once more, same inputs
    res = []
    for p, (send, recv) in zip(plans[1:], bufs[1:]):
        for t in dsts:
            t.zero_()
        p.pack_many(sp)
        p.local_many(sp, dp)
        p.unpack_many(dp)
        torch.cuda.synchronize()
        res.append([send.clone()] + [t.clone() for t in dsts])
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
               for x, y in zip(*res))
    out(f"{name} (c) staging and destinations == (b), byte for byte: {same}")
    for p in plans:
        p.set_buffers(0, 0)
    if not same:
        sys.exit("grouped wire output differs from the ungrouped one")


def run_world1(name, N, elem, reps, warmup, out):
    tdt, ssz, code, wsz = elem
    dims = (N,) * 3
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    pa = native.NativePlan(Pi, Po, 0, ssz)
    pb = native.NativePlan(Pi, Po, 0, ssz, wire=code)
    pc = native.NativePlan(Pi, Po, 0, ssz, wire=code, group_cvt=True)
    plans = (pa, pb, pc)
    src = torch.randn(Pi.length_local(0), dtype=tdt, device="cuda:0")
    ds = [torch.zeros_like(src) for _ in plans]
    st = abc([(lambda p=p, d=d: p.execute(src.data_ptr(), d.data_ptr(), 0))
              for p, d in zip(plans, ds)], reps, warmup)
    nbytes = 2 * ssz * src.numel()
    sp, dp = [src.data_ptr()], [ds[0].data_ptr()]
    out(line(name, "whole", st, (nbytes,) * 3,
             [kinds_of(p.stage_launches(1, native.STAGE_LOCAL, sp, dp))
              for p in plans]))
    # the wire result is the ordinary one, rounded; (c) is (b)
    same = torch.equal(ds[1], ds[0].to(torch.float32).to(tdt)) \
        if code == native.WIRE_F64_F32 else None
    out(f"{name} wire output == round(ordinary output): {same}")
    same_c = torch.equal(ds[2].view(torch.uint8), ds[1].view(torch.uint8))
    out(f"{name} (c) output == (b), byte for byte: {same_c}")
    if same is False or not same_c:
        sys.exit("wire output differs from the rounded ordinary output")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", type=int, default=None)
    args = ap.parse_args()
    if args.reps < 15:
        sys.exit("--reps must be >= 15")

    if args.case is not None:
        if not torch.cuda.is_available():
            sys.exit("wire_bench needs a ROCm GPU")
        name, kind, N, n, elem = CASES[args.case]
        def out(s):
            print(s, flush=True)
        if kind == "slab":
            run_slab(name, N, n, elem, args.reps, args.warmup, out)
        else:
            run_world1(name, N, elem, args.reps, args.warmup, out)
        return

    lines = [
        f"# tools/wire_bench.py; rank 0; median of {args.reps} (min..max), "
        f"us; (a)/(b)/(c) alternating in one process per case, HIP events "
        f"around the whole stage; GB/s = bytes read + written / median",
        "# (a) ordinary = the plan without a wire pair; (b) wire = NARROW "
        "packs, ROUND local, WIDEN unpacks, one launch per descriptor; (c) = "
        "(b) created with PA_PLAN_GROUP_CVT; the exchange is not run (one "
        "GPU)",
        "# c<=b / c<=a: met = (c)'s median at or below the other's, or the "
        "min..max ranges overlap",
    ]
    print("\n".join(lines), flush=True)
    for i in range(len(CASES)):
        r = subprocess.run(
            ["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable,
             os.path.abspath(__file__), "--case", str(i), "--reps",
             str(args.reps), "--warmup", str(args.warmup)],
            stdout=subprocess.PIPE, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            sys.exit(f"case {i} ({CASES[i][0]}) ended with status "
                     f"{r.returncode}: stopping")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
