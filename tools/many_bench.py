"""Pack and unpack stages of a multi-field transpose, per-descriptor launches
against the grouped stage call, on one GPU.

For simulated rank 0 of an (8,) slab x->y at 256^3 and 512^3 and of a (2,4)
grid y->z at 512^3 (f64, permuted output pencils) and n = 1 and 3 fields:

  (a) loop: one pa_device_copy per descriptor — the launches
      pa_transpose_execute makes, per field;
  (b) grouped: pa_transpose_pack_many / pa_transpose_unpack_many.

Both run in ONE process, alternating a, b, a, b, ..., each sample timed with
HIP events around the whole stage, after a warm-up of every shape.  Reported:
median of REPS samples with min..max, the launches each side makes, and the
bytes the stage moves (read + written) over the median.  (a) and (b) are
also compared byte for byte at every shape.

    python tools/many_bench.py [--out profiles/many_bench.txt] [--reps 21]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, build_plan, native  # noqa: E402
from pencilarrays_amd.plan import copydesc_many  # noqa: E402

ESZ = 8
CASES = [
    # name, dims, pdims, (decomp_in, perm_in), (decomp_out, perm_out)
    ("slab8 x->y 256^3", (256,) * 3, (8,), ((1,), None), ((0,), (1, 0, 2))),
    ("slab8 x->y 512^3", (512,) * 3, (8,), ((1,), None), ((0,), (1, 0, 2))),
    ("2x4  y->z 512^3", (512,) * 3, (2, 4), ((0, 2), (1, 2, 0)),
     ((0, 1), (2, 1, 0))),
]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("many_bench needs a ROCm GPU")
    if args.reps < 15:
        sys.exit("--reps must be >= 15")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/many_bench.py on {torch.cuda.get_device_name(0)}; f64; "
        f"rank 0; median of {args.reps} (min..max), us; a/b alternating in "
        f"one process, HIP events around the whole stage")
    out("# loop = one pa_device_copy per descriptor; grouped = "
        "pa_transpose_{pack,unpack}_many")
    for name, dims, pdims, (di, pi), (do, po) in CASES:
        topo = Topology(pdims)
        Pi = Pencil(topo, dims, di, permute=pi)
        Po = Pencil(topo, dims, do, permute=po)
        pyp = build_plan(Pi, Po, 0)
        for n in (1, 3):
            pl = native.NativePlan(Pi, Po, 0, ESZ)
            sb, rb = pl.buffer_sizes_many(n)
            srcs = [torch.randn(Pi.length_local(0), dtype=torch.float64,
                                device="cuda:0") for _ in range(n)]
            send = torch.zeros(sb // ESZ, dtype=torch.float64,
                               device="cuda:0")
            send_b = torch.zeros_like(send)
            recv = torch.randn(rb // ESZ, dtype=torch.float64,
                               device="cuda:0")
            dsts = [torch.zeros(Po.length_local(0), dtype=torch.float64,
                                device="cuda:0") for _ in range(n)]
            dsts_b = [torch.zeros_like(d) for d in dsts]
            sp = [t.data_ptr() for t in srcs]
            dp = [t.data_ptr() for t in dsts_b]
            pl.set_buffers(send_b.data_ptr(), recv.data_ptr())
            packs = [(copydesc_many(pyp, n, f, 1, b.peer_k), f)
                     for f in range(n) for b in pyp.peers
                     if b.pack is not None]
            unpacks = [(copydesc_many(pyp, n, f, 2, b.peer_k), f)
                       for f in range(n) for b in pyp.peers
                       if b.unpack is not None]

            def pack_loop():
                for d, f in packs:
                    native.device_copy(d, ESZ, sp[f], send.data_ptr())

            def unpack_loop():
                for d, f in unpacks:
                    native.device_copy(d, ESZ, recv.data_ptr(),
                                       dsts[f].data_ptr())

            stages = [
                ("pack", pack_loop, lambda: pl.pack_many(sp),
                 native.STAGE_PACK, len(packs),
                 sum(d.nelem for d, _ in packs)),
                ("unpack", unpack_loop, lambda: pl.unpack_many(dp),
                 native.STAGE_UNPACK, len(unpacks),
                 sum(d.nelem for d, _ in unpacks)),
            ]
            for sname, fa, fb, stage, nloop, nelem in stages:
                for _ in range(args.warmup):
                    fa()
                    fb()
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(args.reps):
                    ta.append(timed(fa))
                    tb.append(timed(fb))
                torch.cuda.synchronize()
                same = (torch.equal(send, send_b) if sname == "pack" else
                        all(torch.equal(x, y) for x, y in zip(dsts, dsts_b)))
                rows = pl.stage_launches(n, stage, sp, dp)
                kinds = "+".join(
                    f"{native.KERNEL_NAMES[r.kind]}"
                    f"{'[g' + str(r.entries) + ']' if r.grouped else ''}"
                    for r in rows)
                ma, la, ha = stats(ta)
                mb, lb, hb = stats(tb)
                gb = 2 * nelem * ESZ / 1e9
                out(f"{name} n={n} {sname:6s} "
                    f"loop {nloop:2d} launches {ma:8.1f} ({la:.1f}..{ha:.1f})"
                    f" {gb / (ma * 1e-6):6.0f} GB/s | grouped {len(rows)} "
                    f"launch {kinds} {mb:8.1f} ({lb:.1f}..{hb:.1f}) "
                    f"{gb / (mb * 1e-6):6.0f} GB/s | grouped/loop "
                    f"{mb / ma:.3f} | outputs "
                    f"{'identical' if same else 'DIFFER'}")
                if not same:
                    sys.exit("grouped stage output differs from the loop")
            pl.set_buffers(0, 0)
            del srcs, send, send_b, recv, dsts, dsts_b
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
