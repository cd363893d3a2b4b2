"""Destination-side stages of a scaled transpose against the ordinary plan's,
on one GPU.

Cases: a world-1 512^3 permuted x->y transpose of f64 and of c128 and an
unpermuted one of f64 (the local stage is the whole transpose; unpermuted it
is one linear run), and simulated rank 0 of an (8,) slab at 256^3
and 512^3 with 3 f64 fields (local and unpack stages).  Each stage is timed
three ways:

  (a) ordinary: the plan without a scale — code this feature does not touch,
      the yardstick;
  (b) scaled:   the scaled plan's stage (pa_plan_set_scale, alpha = 1/N);
  (c) a + mul_: (a)'s stage followed by an in-place multiply of every whole
      destination — what a user does today to get the same result.

All run in ONE process, alternating a, b, c, a, b, c, ..., each sample timed
with HIP events around the whole stage, after a warm-up of every shape.
Reported: median of REPS samples with min..max and the launches of (a) and
(b).  The staging buffers hold arbitrary data (the exchange itself cannot run
on one GPU); results are checked by the tests, not here.

    python tools/scale_bench.py [--out profiles/scale_bench.txt] [--reps 21]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, native  # noqa: E402

X1 = ((1, 2), None)
Y1 = ((0, 2), (1, 2, 0))
XS = ((1,), None)
YS = ((0,), (1, 0, 2))


def cases():
    """(name, dims, pdims, in, out, real scalars per element, fields,
    stages)"""
    loc, unp = ("local", native.STAGE_LOCAL), ("unpack", native.STAGE_UNPACK)
    out = [("world1 x->y 512^3 f64", (512,) * 3, (1, 1), X1, Y1, 1, 1, [loc]),
           ("world1 x->y 512^3 c128", (512,) * 3, (1, 1), X1, Y1, 2, 1,
            [loc]),
           # no permutation: the local copy is one run (the linear kernels)
           ("world1 x->y 512^3 f64 unpermuted", (512,) * 3, (1, 1), X1,
            ((0, 2), None), 1, 1, [loc])]
    for N in (256, 512):
        out.append((f"slab8 rank0 x->y {N}^3 f64", (N,) * 3, (8,), XS, YS, 1,
                    3, [loc, unp]))
    return out


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def fmt(xs):
    return f"{statistics.median(xs):8.1f} ({min(xs):.1f}..{max(xs):.1f})"


def kinds(rows):
    return "+".join(
        f"{native.KERNEL_NAMES[r.kind]}"
        f"{'[g' + str(r.entries) + ']' if r.grouped else ''}"
        for r in rows) or "none"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scale_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/scale_bench.py on {torch.cuda.get_device_name(0)}; median "
        f"of {args.reps} (min..max), us; a/b/c alternating in one process, "
        f"HIP events around the whole stage")
    out("# a = ordinary plan's stage; b = scaled plan's stage; c = a + "
        "in-place mul_ of every whole destination")
    met = []
    for name, dims, pdims, (di, pi), (do, po), nscal, n, stages in cases():
        topo = Topology(pdims)
        Pi = Pencil(topo, dims, di, permute=pi)
        Po = Pencil(topo, dims, do, permute=po)
        alpha = 1.0 / (dims[0] * dims[1] * dims[2])
        stream = torch.cuda.current_stream().cuda_stream
        plans = [native.NativePlan(Pi, Po, 0, 8 * nscal),
                 native.NativePlan(Pi, Po, 0, 8 * nscal)]
        plans[1].set_scale(native.SCALAR_F64, alpha)
        sb, rb = plans[0].buffer_sizes_many(n)
        assert (sb, rb) == plans[1].buffer_sizes_many(n)
        srcs = [torch.randn(Pi.length_local(0) * nscal, dtype=torch.float64,
                            device="cuda:0") for _ in range(n)]
        dsts = [torch.zeros(Po.length_local(0) * nscal, dtype=torch.float64,
                            device="cuda:0") for _ in range(n)]
        send = torch.zeros(max(sb, 8) // 8, dtype=torch.float64,
                           device="cuda:0")
        recv = torch.randn(max(rb, 8) // 8, dtype=torch.float64,
                           device="cuda:0")
        for p in plans:
            p.set_buffers(send.data_ptr(), recv.data_ptr())
        sp = [t.data_ptr() for t in srcs]
        dp = [t.data_ptr() for t in dsts]

        def stage_fn(p, sname):
            if sname == "local":
                return lambda: p.local_many(sp, dp, stream)
            return lambda: p.unpack_many(dp, stream)

        out(f"{name} n={n} alpha=1/{dims[0]}^3 destination "
            f"{dsts[0].numel() * 8 * n / 2 ** 20:.0f} MiB")
        for sname, stage in stages:
            fa, fb = stage_fn(plans[0], sname), stage_fn(plans[1], sname)

            def fc():
                fa()
                for t in dsts:
                    t.mul_(alpha)

            for _ in range(args.warmup):
                fa()
                fb()
                fc()
            torch.cuda.synchronize()
            ta, tb, tc = [], [], []
            for _ in range(args.reps):
                ta.append(timed(fa))
                tb.append(timed(fb))
                tc.append(timed(fc))
            torch.cuda.synchronize()
            ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
            ok = mc - mb > max(tc) - min(tc)
            met.append(ok)
            out(f"  {sname:6s} a {fmt(ta)} {kinds(plans[0].stage_launches(n, stage, sp, dp))}"
                f" | b {fmt(tb)} {kinds(plans[1].stage_launches(n, stage, sp, dp))}"
                f" | c {fmt(tc)} | b/a {mb / ma:.3f} | b/c {mb / mc:.3f} | "
                f"b below c by more than c's spread: "
                f"{'met' if ok else 'NOT met'}")
        for p in plans:
            p.set_buffers(0, 0)
        del srcs, dsts, send, recv
        torch.cuda.empty_cache()
    out(f"# b below c by more than c's min..max spread: "
        f"{sum(met)} of {len(met)} stages")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
