"""Grouped and truncated split / join stages on one GPU.

Simulated rank 0 of an (8,) slab, n = 3 components, f64 and f32, 256^3 and
512^3, permuted output pencils.

  (i)  grouping alone, x->y: the split / join stages of an ordinary plan
       created with PA_PLAN_GROUP_SOA (a) against the same plan without the
       flag (b), which launches once per block: the split's pack, the join's
       unpack, and "both" (the pack then the unpack in one timed region).
  (ii) the feature, y->z with the 2/3-rule keep set on two dims
       (fourier_keep): the truncated split stages (pack + local) and the
       truncated, scaled join stages (local + unpack) with fill = zero (a)
       against what a user does today (b), code this change does not touch:
       the n-field keep plan's stages plus ONE torch copy_ between the
       vector-valued array and the fields (before the stage for a split,
       after it for a join) plus, for the scaled join, an in-place mul_ of
       the vector-valued array.  As in tools/soa_bench.py a user runs the
       torch passes once per hop, so the per-stage rows of (b) each carry
       them and "both" times the two stages with the passes once.

All run in ONE process, legs alternating a, b, a, b, ..., each sample timed
with HIP events around the whole stage, after a warm-up of every shape.
Reported: median of REPS samples with min..max.  Staging holds arbitrary data
(the exchange itself cannot run on one GPU); results are checked by the
tests, not here.

    python tools/soa_group_bench.py [--out profiles/soa_group_bench.txt]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, fourier_keep, native  # noqa: E402

X = ((1,), None)
Y = ((0,), (1, 0, 2))
Z = ((1,), (2, 1, 0))
N = 3
TYPES = [("f64", 8, torch.float64, native.SCALAR_F64),
         ("f32", 4, torch.float32, native.SCALAR_F32)]
SPLIT, JOIN = native.SOA_SPLIT, native.SOA_JOIN


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


def launches(rows):
    return sum(1 if r.grouped else r.entries for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("soa_group_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    def measure(label, fa, fb, claim):
        """alternate a and b; claim "below": a below b by more than b's
        spread; "not_above": a not above b by more than b's spread"""
        for _ in range(args.warmup):
            fa()
            fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(fa))
            tb.append(timed(fb))
        torch.cuda.synchronize()
        ma, mb = statistics.median(ta), statistics.median(tb)
        spread = max(tb) - min(tb)
        below = mb - ma > spread
        not_above = ma - mb <= spread
        out(f"  {label:22s} a {fmt(ta)} | b {fmt(tb)} | a/b {ma / mb:.3f} | "
            f"a below b by more than b's spread: "
            f"{'met' if below else 'NOT met'}; a not above b by more than "
            f"b's spread: {'met' if not_above else 'NOT met'}")
        return below if claim == "below" else not_above

    out(f"# tools/soa_group_bench.py on {torch.cuda.get_device_name(0)}; "
        f"rank 0 of an (8,) slab; n = {N}; median of {args.reps} "
        f"(min..max), us; a/b alternating in one process, HIP events around "
        f"the whole stage")
    stream = torch.cuda.current_stream().cuda_stream
    topo = Topology((8,))
    met = {}

    def rnd(count, ssz, dt):
        return torch.randint(0, 255, (count * ssz,), dtype=torch.uint8,
                             device="cuda:0").view(dt)

    out("# (i) grouping alone, x->y: a = PA_PLAN_GROUP_SOA, b = the same "
        "plan without the flag")
    for size in args.sizes:
        dims = (size,) * 3
        Pi = Pencil(topo, dims, X[0], permute=X[1])
        Po = Pencil(topo, dims, Y[0], permute=Y[1])
        Li, Lo = Pi.length_local(0), Po.length_local(0)
        for tname, ssz, dt, _ in TYPES:
            flat = native.NativePlan(Pi, Po, 0, ssz)
            grp = native.NativePlan(Pi, Po, 0, ssz, group_soa=True)
            sb, rb = flat.buffer_sizes_many(N)
            send = torch.zeros(max(sb, 16), dtype=torch.uint8, device="cuda:0")
            recv = torch.randint(0, 255, (max(rb, 16),), dtype=torch.uint8,
                                 device="cuda:0")
            for p in (flat, grp):
                p.set_buffers(send.data_ptr(), recv.data_ptr())
            aos_i, aos_o = rnd(Li * N, ssz, dt), rnd(Lo * N, ssz, dt)
            ai, ao = aos_i.data_ptr(), aos_o.data_ptr()
            la = [launches(p.stage_launches_soa(N, SPLIT, native.STAGE_PACK,
                                                ai)) for p in (grp, flat)]
            lb = [launches(p.stage_launches_soa(N, JOIN, native.STAGE_UNPACK,
                                                ao)) for p in (grp, flat)]
            out(f"slab8 x->y {size}^3 {tname} x {N}: launches a/b: pack "
                f"{la[0]}/{la[1]}, unpack {lb[0]}/{lb[1]}")
            claim = "below" if size <= 256 else "not_above"
            for label, mk in (
                    ("split pack", lambda p: lambda: p.pack_split(
                        N, ai, stream)),
                    ("join unpack", lambda p: lambda: p.unpack_join(
                        N, ao, stream)),
                    ("both", lambda p: lambda: (
                        p.pack_split(N, ai, stream),
                        p.unpack_join(N, ao, stream)))):
                ok = measure(label, mk(grp), mk(flat), claim)
                met.setdefault(("i", size, claim), []).append(ok)
            for p in (flat, grp):
                p.set_buffers(0, 0)
            del aos_i, aos_o, send, recv
            torch.cuda.empty_cache()

    out("# (ii) truncated split and scaled join, y->z, 2/3 rule on dims 0 "
        "and 1, fill = zero: a = split / join on the flagged keep plan, b = "
        "the n-field keep plan's stages + one torch copy_ (+ mul_ for the "
        "join)")
    for size in args.sizes:
        dims = (size,) * 3
        keep = fourier_keep(dims, [2 * size // 3 - 1, size // 3, None],
                            real_dim=0)
        Pi = Pencil(topo, dims, Y[0], permute=Y[1])
        Po = Pencil(topo, dims, Z[0], permute=Z[1])
        Li, Lo = Pi.length_local(0), Po.length_local(0)
        alpha = 1.0 / size ** 3
        for tname, ssz, dt, code in TYPES:
            many = native.NativePlan(Pi, Po, 0, ssz, keep=keep)
            grp = native.NativePlan(Pi, Po, 0, ssz, keep=keep, group_soa=True)
            full = native.NativePlan(Pi, Po, 0, ssz)
            sb, rb = many.buffer_sizes_many(N)
            fs, fr = full.buffer_sizes_many(N)
            send = torch.zeros(max(sb, 16), dtype=torch.uint8, device="cuda:0")
            recv = torch.randint(0, 255, (max(rb, 16),), dtype=torch.uint8,
                                 device="cuda:0")
            for p in (many, grp):
                p.set_buffers(send.data_ptr(), recv.data_ptr())
            aos_i, soa_i = rnd(Li * N, ssz, dt), rnd(Li * N, ssz,
                                                     dt).view(N, Li)
            aos_o, soa_o = rnd(Lo * N, ssz, dt), rnd(Lo * N, ssz,
                                                     dt).view(N, Lo)
            fi = [soa_i[c].data_ptr() for c in range(N)]
            fo = [soa_o[c].data_ptr() for c in range(N)]
            ai, ao = aos_i.data_ptr(), aos_o.data_ptr()
            rows = {
                "pack": grp.stage_launches_soa(N, SPLIT, native.STAGE_PACK,
                                               ai),
                "local": grp.stage_launches_soa(N, JOIN, native.STAGE_LOCAL,
                                                ao, fi),
                "unpack": grp.stage_launches_soa(N, JOIN, native.STAGE_UNPACK,
                                                 ao),
            }
            out(f"slab8 y->z {size}^3 {tname} x {N} keep={keep}: staged "
                f"bytes kept {sb / max(fs, 1):.3f} (send) "
                f"{rb / max(fr, 1):.3f} (recv); launches of a: "
                + ", ".join(f"{k} {launches(v)} ({sum(r.entries for r in v)} "
                            f"entries)" for k, v in rows.items()))

            def deinterleave():   # vector-valued source -> the n fields
                soa_i.copy_(aos_i.view(Li, N).t())

            def interleave():     # the n fields -> vector-valued destination
                aos_o.view(Lo, N).copy_(soa_o.t())

            def scale():
                aos_o.mul_(alpha)

            cases = [
                ("split pack",
                 lambda: grp.pack_split(N, ai, stream),
                 lambda: (deinterleave(), many.pack_many(fi, stream))),
                ("split local",
                 lambda: grp.local_split(ai, fo, stream),
                 lambda: (deinterleave(), many.local_many(fi, fo, stream))),
                ("split both",
                 lambda: (grp.pack_split(N, ai, stream),
                          grp.local_split(ai, fo, stream)),
                 lambda: (deinterleave(), many.pack_many(fi, stream),
                          many.local_many(fi, fo, stream))),
                ("join local scaled",
                 lambda: grp.local_join_scaled(code, alpha, fi, ao, stream),
                 lambda: (many.local_many(fi, fo, stream), interleave(),
                          scale())),
                ("join unpack scaled",
                 lambda: grp.unpack_join_scaled(N, code, alpha, ao, stream),
                 lambda: (many.unpack_many(fo, stream), interleave(),
                          scale())),
                ("join both scaled",
                 lambda: (grp.local_join_scaled(code, alpha, fi, ao, stream),
                          grp.unpack_join_scaled(N, code, alpha, ao, stream)),
                 lambda: (many.local_many(fi, fo, stream),
                          many.unpack_many(fo, stream), interleave(),
                          scale())),
            ]
            for label, fa, fb in cases:
                ok = measure(label, fa, fb, "below")
                met.setdefault(("ii", size, "below"), []).append(ok)
            for p in (many, grp):
                p.set_buffers(0, 0)
            del aos_i, soa_i, aos_o, soa_o, send, recv
            torch.cuda.empty_cache()

    for (which, size, claim), oks in sorted(met.items()):
        what = "a below b by more than b's min..max spread" \
            if claim == "below" else \
            "a not above b by more than b's min..max spread"
        out(f"# ({which}) {size}^3: {what}: {sum(oks)} of {len(oks)} rows")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
