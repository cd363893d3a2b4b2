"""Scaled split and join stages against what a user does today, on one GPU.

Cases: n = 3 components of f64, f32 and complex128; a world-1 512^3 permuted
x->y transpose (the local stage is the whole transpose) and simulated rank 0
of an (8,) slab at 512^3.  A scaled split multiplies in its pack and local
stages, a scaled join in its local and unpack stages.  Each such stage is
timed three ways:

  (a) scaled:   the *_scaled stage, the 1/N folded into the layout change;
  (b) today:    the unscaled split / join stage (the code path the scaled
      calls leave untouched) followed by ONE in-place torch mul_ on the real
      view of what the stage wrote: the send buffer for pack_split, the n
      fields for local_split, the vector-valued array for the join stages;
  (c) unscaled: the unscaled stage alone -- what the multiply costs on top.

On the slab a join's two stages write parts of ONE array, and a user runs the
mul_ of (b) once per hop, not once per stage: the per-stage join rows of the
slab each carry that whole-array pass.  The row "both" times the two stages
together with each mul_ once; it is the one to read for a hop.

All run in ONE process, alternating a, b, c, a, b, c, ..., each sample timed
with HIP events around the whole stage, after a warm-up of every shape.
Reported: median of REPS samples with min..max.  The staging buffers hold
arbitrary data (the exchange itself cannot run on one GPU); results are
checked by the tests, not here.

    python tools/soa_scale_bench.py [--out profiles/soa_scale_bench.txt]
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
N = 3
# name, scalar bytes, array dtype, real dtype, PA_SCALAR code
TYPES = [("f64", 8, torch.float64, torch.float64, native.SCALAR_F64),
         ("f32", 4, torch.float32, torch.float32, native.SCALAR_F32),
         ("c128", 16, torch.complex128, torch.float64, native.SCALAR_F64)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("soa_scale_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    alpha = 1.0 / args.size ** 3
    out(f"# tools/soa_scale_bench.py on {torch.cuda.get_device_name(0)}; "
        f"n = {N}; alpha = 1/{args.size}^3; median of {args.reps} "
        f"(min..max), us; a/b/c alternating in one process, HIP events "
        f"around the whole stage")
    out("# a = scaled split / join stage; b = unscaled stage + one in-place "
        "torch mul_ on the real view of what it wrote; c = unscaled stage "
        "alone")
    met, ac_out = [], []
    dims = (args.size,) * 3
    shapes = [(f"world1 x->y {args.size}^3", (1, 1), X1, Y1,
               {"split": ["local"], "join": ["local"]}),
              (f"slab8 rank0 x->y {args.size}^3", (8,), XS, YS,
               {"split": ["pack", "local"], "join": ["local", "unpack"]})]
    stream = torch.cuda.current_stream().cuda_stream
    for tname, ssz, dt, rdt, code in TYPES:
        rsz = torch.empty((), dtype=rdt).element_size()
        for sname, pdims, (di, pi), (do, po), stages in shapes:
            topo = Topology(pdims)
            Pi = Pencil(topo, dims, di, permute=pi)
            Po = Pencil(topo, dims, do, permute=po)
            Li, Lo = Pi.length_local(0), Po.length_local(0)
            p = native.NativePlan(Pi, Po, 0, ssz)
            sb, rb = p.buffer_sizes_many(N)
            send = torch.zeros(max(sb, 16), dtype=torch.uint8, device="cuda:0")
            recv = torch.rand(max(rb, 16) // rsz, dtype=rdt,
                              device="cuda:0").view(torch.uint8)
            p.set_buffers(send.data_ptr(), recv.data_ptr())
            send_real = send[:sb - sb % rsz].view(rdt)

            def rnd(count):   # finite values, so that mul_ sees plain data
                return torch.rand(count * ssz // rsz, dtype=rdt,
                                  device="cuda:0").view(dt)

            aos_i = rnd(Li * N)
            aos_o, soa_i, soa_o = rnd(Lo * N), rnd(Li * N).view(N, Li), \
                rnd(Lo * N).view(N, Lo)
            fi = [soa_i[c].data_ptr() for c in range(N)]
            fo = [soa_o[c].data_ptr() for c in range(N)]
            ai, ao = aos_i.data_ptr(), aos_o.data_ptr()
            aos_o_real, soa_o_real = aos_o.view(rdt), soa_o.view(rdt)
            out(f"{sname} {tname} x {N}: vector field "
                f"{Li * N * ssz / 2 ** 20:.0f} MiB in, "
                f"{Lo * N * ssz / 2 ** 20:.0f} MiB out")

            legs = {
                ("split", "pack"): (
                    lambda: p.pack_split_scaled(N, code, alpha, ai, stream),
                    lambda: (p.pack_split(N, ai, stream),
                             send_real.mul_(alpha)),
                    lambda: p.pack_split(N, ai, stream)),
                ("split", "local"): (
                    lambda: p.local_split_scaled(code, alpha, ai, fo, stream),
                    lambda: (p.local_split(ai, fo, stream),
                             soa_o_real.mul_(alpha)),
                    lambda: p.local_split(ai, fo, stream)),
                ("join", "local"): (
                    lambda: p.local_join_scaled(code, alpha, fi, ao, stream),
                    lambda: (p.local_join(fi, ao, stream),
                             aos_o_real.mul_(alpha)),
                    lambda: p.local_join(fi, ao, stream)),
                ("join", "unpack"): (
                    lambda: p.unpack_join_scaled(N, code, alpha, ao, stream),
                    lambda: (p.unpack_join(N, ao, stream),
                             aos_o_real.mul_(alpha)),
                    lambda: p.unpack_join(N, ao, stream)),
            }
            # the two multiplying stages of a slab hop together, with every
            # mul_ of (b) ONCE, as a user runs it
            hops = {
                "split": (
                    lambda: (p.pack_split_scaled(N, code, alpha, ai, stream),
                             p.local_split_scaled(code, alpha, ai, fo,
                                                  stream)),
                    lambda: (p.pack_split(N, ai, stream),
                             p.local_split(ai, fo, stream),
                             send_real.mul_(alpha), soa_o_real.mul_(alpha)),
                    lambda: (p.pack_split(N, ai, stream),
                             p.local_split(ai, fo, stream))),
                "join": (
                    lambda: (p.local_join_scaled(code, alpha, fi, ao, stream),
                             p.unpack_join_scaled(N, code, alpha, ao,
                                                  stream)),
                    lambda: (p.local_join(fi, ao, stream),
                             p.unpack_join(N, ao, stream),
                             aos_o_real.mul_(alpha)),
                    lambda: (p.local_join(fi, ao, stream),
                             p.unpack_join(N, ao, stream))),
            }
            for which in ("split", "join"):
                rows = list(stages[which])
                if len(rows) > 1:
                    rows.append("both")
                for stage in rows:
                    fa, fb, fc = hops[which] if stage == "both" else \
                        legs[(which, stage)]
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
                    ok = mb - ma > max(tb) - min(tb)
                    inside = min(tc) <= ma <= max(tc)
                    if stage != "both":  # the counts are per stage
                        met.append(ok)
                        ac_out.append(not inside)
                    out(f"  {which:5s} {stage:6s} a {fmt(ta)} | b {fmt(tb)} | "
                        f"c {fmt(tc)} | a/b {ma / mb:.3f} | a/c "
                        f"{ma / mc:.3f} ({'inside' if inside else 'OUTSIDE'} "
                        f"c's spread) | a below b by more than b's spread: "
                        f"{'met' if ok else 'NOT met'}")
            p.set_buffers(0, 0)
            del aos_i, soa_i, aos_o, soa_o, send, recv, send_real
            del aos_o_real, soa_o_real
            torch.cuda.empty_cache()
    out(f"# a below b by more than b's min..max spread: "
        f"{sum(met)} of {len(met)} stages")
    out(f"# a outside c's min..max spread: {sum(ac_out)} of {len(ac_out)} "
        f"stages")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
