"""Split and join stages against what a user does today, on one GPU.

Cases: n = 3 components of f64, f32 and complex128; a world-1 512^3 permuted
x->y transpose (the local stage is the whole transpose) and simulated rank 0
of an (8,) slab at 512^3 (a split changes the layout in its pack and local
stages, a join in its local and unpack stages).  Each such stage is timed
three ways:

  (a) split / join: the new stage, the vector-valued array on one side;
  (b) today:        the n-field plan's stage (pa_transpose_*_many, code this
      feature does not touch) plus the torch pass between the vector-valued
      array and the n fields -- ONE strided copy_ over the whole field, the
      fields being the rows of one (n, L) tensor: before the stage for a
      split, after it for a join;
  (c) wide element: the same stage of the ordinary elem_dims = (3,) plan
      (PA_KERNEL_TILE_WIDE where permuted), which moves the same bytes and
      changes no layout -- the byte-equal yardstick.

On the slab a hop has two layout-changing stages, and a user runs the torch
pass of (b) once per hop, not once per stage: the per-stage rows of the slab
each carry that whole-field pass, so their a/b counts it twice per hop.  The
row "both" times the two stages together with the pass once; it is the one
to read for a hop.

All run in ONE process, alternating a, b, c, a, b, c, ..., each sample timed
with HIP events around the whole stage, after a warm-up of every shape.
Reported: median of REPS samples with min..max.  The staging buffers hold
arbitrary data (the exchange itself cannot run on one GPU); results are
checked by the tests, not here.

    python tools/soa_bench.py [--out profiles/soa_bench.txt] [--reps 21]
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
TYPES = [("f64", 8, torch.float64), ("f32", 4, torch.float32),
         ("c128", 16, torch.complex128)]


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
        sys.exit("soa_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/soa_bench.py on {torch.cuda.get_device_name(0)}; n = {N}; "
        f"median of {args.reps} (min..max), us; a/b/c alternating in one "
        f"process, HIP events around the whole stage")
    out("# a = split / join stage; b = n-field stage + one torch copy_ "
        "between the vector-valued array and the fields; c = the "
        "elem_dims=(3,) plan's stage")
    met = []
    dims = (args.size,) * 3
    shapes = [(f"world1 x->y {args.size}^3", (1, 1), X1, Y1,
               {"split": ["local"], "join": ["local"]}),
              (f"slab8 rank0 x->y {args.size}^3", (8,), XS, YS,
               {"split": ["pack", "local"], "join": ["local", "unpack"]})]
    stream = torch.cuda.current_stream().cuda_stream
    for tname, ssz, dt in TYPES:
        for sname, pdims, (di, pi), (do, po), stages in shapes:
            topo = Topology(pdims)
            Pi = Pencil(topo, dims, di, permute=pi)
            Po = Pencil(topo, dims, do, permute=po)
            Li, Lo = Pi.length_local(0), Po.length_local(0)
            scalar = native.NativePlan(Pi, Po, 0, ssz)
            wide = native.NativePlan(Pi, Po, 0, ssz, ncomp=N)
            sb, rb = scalar.buffer_sizes_many(N)
            assert (sb, rb) == wide.buffer_sizes_many(1)
            send = torch.zeros(max(sb, 16), dtype=torch.uint8, device="cuda:0")
            recv = torch.randint(0, 255, (max(rb, 16),), dtype=torch.uint8,
                                 device="cuda:0")
            for p in (scalar, wide):
                p.set_buffers(send.data_ptr(), recv.data_ptr())

            def rnd(count):
                return torch.randint(0, 255, (count * ssz,),
                                     dtype=torch.uint8,
                                     device="cuda:0").view(dt)

            # input side and output side, each in both forms
            aos_i, soa_i = rnd(Li * N), rnd(Li * N).view(N, Li)
            aos_o, soa_o = rnd(Lo * N), rnd(Lo * N).view(N, Lo)
            fi = [soa_i[c].data_ptr() for c in range(N)]
            fo = [soa_o[c].data_ptr() for c in range(N)]
            ai, ao = aos_i.data_ptr(), aos_o.data_ptr()
            out(f"{sname} {tname} x {N}: vector field "
                f"{Li * N * ssz / 2 ** 20:.0f} MiB in, "
                f"{Lo * N * ssz / 2 ** 20:.0f} MiB out")

            def deinterleave():   # vector-valued source -> the n fields
                soa_i.copy_(aos_i.view(Li, N).t())

            def interleave():     # the n fields -> vector-valued destination
                aos_o.view(Lo, N).copy_(soa_o.t())

            legs = {
                ("split", "pack"): (
                    lambda: scalar.pack_split(N, ai, stream),
                    lambda: (deinterleave(), scalar.pack_many(fi, stream)),
                    lambda: wide.pack_many([ai], stream)),
                ("split", "local"): (
                    lambda: scalar.local_split(ai, fo, stream),
                    lambda: (deinterleave(),
                             scalar.local_many(fi, fo, stream)),
                    lambda: wide.local_many([ai], [ao], stream)),
                ("join", "local"): (
                    lambda: scalar.local_join(fi, ao, stream),
                    lambda: (scalar.local_many(fi, fo, stream),
                             interleave()),
                    lambda: wide.local_many([ai], [ao], stream)),
                ("join", "unpack"): (
                    lambda: scalar.unpack_join(N, ao, stream),
                    lambda: (scalar.unpack_many(fo, stream), interleave()),
                    lambda: wide.unpack_many([ao], stream)),
            }
            # the two layout-changing stages of a slab hop together, with the
            # torch pass of (b) ONCE, as a user runs it
            hops = {
                "split": (
                    lambda: (scalar.pack_split(N, ai, stream),
                             scalar.local_split(ai, fo, stream)),
                    lambda: (deinterleave(), scalar.pack_many(fi, stream),
                             scalar.local_many(fi, fo, stream)),
                    lambda: (wide.pack_many([ai], stream),
                             wide.local_many([ai], [ao], stream))),
                "join": (
                    lambda: (scalar.local_join(fi, ao, stream),
                             scalar.unpack_join(N, ao, stream)),
                    lambda: (scalar.local_many(fi, fo, stream),
                             scalar.unpack_many(fo, stream), interleave()),
                    lambda: (wide.local_many([ai], [ao], stream),
                             wide.unpack_many([ao], stream))),
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
                    if stage != "both":  # the count is per stage
                        met.append(ok)
                    out(f"  {which:5s} {stage:6s} a {fmt(ta)} | b {fmt(tb)} | "
                        f"c {fmt(tc)} | a/b {ma / mb:.3f} | a/c "
                        f"{ma / mc:.3f} | a below b by more than b's "
                        f"spread: {'met' if ok else 'NOT met'}")
            for p in (scalar, wide):
                p.set_buffers(0, 0)
            del aos_i, soa_i, aos_o, soa_o, send, recv
            torch.cuda.empty_cache()
    out(f"# a below b by more than b's min..max spread: "
        f"{sum(met)} of {len(met)} stages")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
