"""Stages of a truncated transpose against the ordinary plan's, on one GPU.

For simulated rank 0 of an (8,) slab at 256^3 and 512^3 (f64, permuted output
pencils), n = 1 and 3 fields, and two hops — x->y with 2/3 of dim 0 kept and
y->z with 2/3 of dims 0 and 1 kept — each of the pack, local and unpack
stages is timed three ways:

  (a) ordinary: the ordinary plan's pa_transpose_{pack,local,unpack}_many —
      code this feature does not touch, the yardstick;
  (b) keep:     the keep plan's stage (PA_FILL_ZERO; the local stage carries
      the grouped zero fill);
  (c) memset+a: hipMemsetAsync of every whole destination, then (a)'s stage —
      what a user does today to get the same result.  Reported for the local
      stage, where the keep plan has its fill.

All run in ONE process, alternating a, b, c, a, b, c, ..., each sample timed
with HIP events around the whole stage, after a warm-up of every shape.
Reported: median of REPS samples with min..max, the launches of (b), and the
kept fraction of the staged bytes.  The staging buffers hold arbitrary data
(the exchange itself cannot run on one GPU); results are checked by the
tests, not here.

    python tools/keep_bench.py [--out profiles/keep_bench.txt] [--reps 21]
"""

import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, fourier_keep, native  # noqa: E402

ESZ = 8
X = ((1,), None)
Y = ((0,), (1, 0, 2))
Z = ((1,), (2, 1, 0))


def cases():
    out = []
    for N in (256, 512):
        dims = (N,) * 3
        out.append((f"slab8 x->y {N}^3", dims, X, Y,
                    fourier_keep(dims, [2 * N // 3 - 1, None, None],
                                 real_dim=0)))
        out.append((f"slab8 y->z {N}^3", dims, Y, Z,
                    fourier_keep(dims, [2 * N // 3 - 1, N // 3, None],
                                 real_dim=0)))
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
    return (f"{statistics.median(xs):8.1f} ({min(xs):.1f}..{max(xs):.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keep_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_size_t, ctypes.c_void_p]
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/keep_bench.py on {torch.cuda.get_device_name(0)}; f64; "
        f"rank 0 of an (8,) slab; median of {args.reps} (min..max), us; "
        f"a/b/c alternating in one process, HIP events around the whole "
        f"stage")
    out("# a = ordinary plan's stage; b = keep plan's stage (local = copies "
        "+ grouped zero fill); c = hipMemsetAsync of every whole destination "
        "+ a")
    for name, dims, (di, pi), (do, po), keep in cases():
        topo = Topology((8,))
        Pi = Pencil(topo, dims, di, permute=pi)
        Po = Pencil(topo, dims, do, permute=po)
        for n in (1, 3):
            stream = torch.cuda.current_stream().cuda_stream
            plans = [native.NativePlan(Pi, Po, 0, ESZ),
                     native.NativePlan(Pi, Po, 0, ESZ, keep=keep)]
            sizes = [p.buffer_sizes_many(n) for p in plans]
            srcs = [torch.randn(Pi.length_local(0), dtype=torch.float64,
                                device="cuda:0") for _ in range(n)]
            dsts = [[torch.zeros(Po.length_local(0), dtype=torch.float64,
                                 device="cuda:0") for _ in range(n)]
                    for _ in plans]
            staging = []
            for p, (sb, rb) in zip(plans, sizes):
                send = torch.zeros(max(sb, ESZ) // ESZ, dtype=torch.float64,
                                   device="cuda:0")
                recv = torch.randn(max(rb, ESZ) // ESZ, dtype=torch.float64,
                                   device="cuda:0")
                p.set_buffers(send.data_ptr(), recv.data_ptr())
                staging.append((send, recv))
            sp = [t.data_ptr() for t in srcs]
            dp = [[t.data_ptr() for t in row] for row in dsts]

            def memset_a(stage_fn):
                def run():
                    for t in dsts[0]:
                        hip.hipMemsetAsync(t.data_ptr(), 0,
                                           t.numel() * ESZ, stream)
                    stage_fn()
                return run

            def stage_fns(i):
                p = plans[i]
                return {
                    "pack": lambda: p.pack_many(sp, stream),
                    "local": lambda: p.local_many(sp, dp[i], stream),
                    "unpack": lambda: p.unpack_many(dp[i], stream),
                }

            fa, fb = stage_fns(0), stage_fns(1)
            out(f"{name} n={n} keep={keep} staged bytes kept "
                f"{sizes[1][0] / max(sizes[0][0], 1):.3f} (send) "
                f"{sizes[1][1] / max(sizes[0][1], 1):.3f} (recv)")
            tot = {"a": 0.0, "b": 0.0, "c": 0.0}
            for sname, stage in (("pack", native.STAGE_PACK),
                                 ("local", native.STAGE_LOCAL),
                                 ("unpack", native.STAGE_UNPACK)):
                fc = memset_a(fa[sname]) if sname == "local" else None
                for _ in range(args.warmup):
                    fa[sname]()
                    fb[sname]()
                    if fc:
                        fc()
                torch.cuda.synchronize()
                ta, tb, tc = [], [], []
                for _ in range(args.reps):
                    ta.append(timed(fa[sname]))
                    tb.append(timed(fb[sname]))
                    if fc:
                        tc.append(timed(fc))
                torch.cuda.synchronize()
                rows = plans[1].stage_launches(n, stage, sp, dp[1])
                kinds = "+".join(
                    f"{native.KERNEL_NAMES[r.kind]}"
                    f"{'[g' + str(r.entries) + ']' if r.grouped else ''}"
                    for r in rows) or "none"
                ma, mb = statistics.median(ta), statistics.median(tb)
                tot["a"] += ma
                tot["b"] += mb
                tot["c"] += statistics.median(tc) if fc else ma
                out(f"  {sname:6s} a {fmt(ta)} | b {fmt(tb)} {kinds} | b/a "
                    f"{mb / ma:.3f}"
                    + (f" | c {fmt(tc)} | b/c "
                       f"{mb / statistics.median(tc):.3f}" if fc else ""))
            out(f"  sum of medians: a {tot['a']:.1f} | b {tot['b']:.1f} | "
                f"c {tot['c']:.1f} | b/a {tot['b'] / tot['a']:.3f} | b/c "
                f"{tot['b'] / tot['c']:.3f}")
            for p in plans:
                p.set_buffers(0, 0)
            del srcs, dsts, staging
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
