# Time permuted transposes of composite elements (three scalars per element,
# components fastest) standalone via the C ABI + HIP events, variants
# interleaved in one process:
#   (a) wide      the wide-element LDS tile through pa_device_copy_comp
#                 (scalar_size, 3)
#   (b) byteify   the path a plain composite elem_size takes: pa_device_copy
#                 with elem_size = 12 / 24.  With --baseline-lib PATH it runs
#                 in that older build of the library, loaded side by side;
#                 without, in this tree (plain elem_size keeps that path)
#   (c) extra     the same bytes as extra_dims=(3,) of the scalar dtype
#                 (components slowest) on the tuned scalar tile: the yardstick
# Workload: the world-1 x->y transpose with the PencilFFTs output permutation
# (1,2,0) on a 512^3 grid, three float32 (12 B) and three float64 (24 B) per
# element.  Reported: MEDIAN GB/s (2*B bytes per element) with min..max over
# the timed launches of that variant.
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, build_plan, native  # noqa: E402

I64 = ctypes.c_int64
NCOMP = 3


def desc_args(desc, esz):
    nd = len(desc.dims)
    return (nd, (I64 * nd)(*desc.dims), (I64 * nd)(*desc.sstrides),
            I64(desc.soffset), (I64 * nd)(*desc.dstrides), I64(desc.doffset),
            I64(esz))


class Variant:
    def __init__(self, name, fn, args, nbytes, reps, kind):
        self.name, self.fn, self.args = name, fn, args
        self.reps, self.kind = reps, kind
        self.gb = nbytes * 2 / 1e9
        self.ms = []

    def launch(self):
        if self.fn(*self.args) != 0:
            raise RuntimeError(f"{self.name}: device copy failed")

    def timed(self):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        self.launch()
        b.record()
        b.synchronize()
        self.ms.append(a.elapsed_time(b))

    def report(self, label):
        gbs = sorted(self.gb / (m * 1e-3) for m in self.ms)
        med = statistics.median(gbs)
        print(f"{label:26s} {self.name:8s} {self.kind:22s} "
              f"median {med:8.1f} GB/s  min {gbs[0]:8.1f}  max {gbs[-1]:8.1f}"
              f"  ({statistics.median(self.ms):.3f} ms, n={len(self.ms)})",
              flush=True)
        return med, gbs[0], gbs[-1]


def kind_name(k):
    s = f"{native.KERNEL_NAMES[k.kind]}/w{k.word_bytes}"
    if k.words_per_element > 1:
        s += f"/m{k.words_per_element}"
    return s + ("/byteified" if k.byteified else "")


def run_shape(dims, ssz, lib, base, reps):
    dev = "cuda:0"
    B = ssz * NCOMP
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    d_elem = build_plan(Pi, Po, 0).local
    d_extra = build_plan(Pi, Po, 0, (NCOMP,)).local
    n = Pi.length_local(0)
    n0, n1, n2 = dims
    label = "x".join(map(str, dims)) + f" 3x{ssz}B"

    src = torch.empty(n * B, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty(n * B, dtype=torch.uint8, device=dev)
    sp, dp = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr())
    blib = base if base is not None else lib

    vs = [
        Variant("wide", lib.pa_device_copy_comp,
                desc_args(d_elem, ssz) + (I64(NCOMP), sp, dp, None), n * B,
                reps, kind_name(native.copy_kernel_kind(
                    d_elem, ssz, src.data_ptr(), dst.data_ptr(),
                    ncomp=NCOMP))),
        Variant("byteify", blib.pa_device_copy,
                desc_args(d_elem, B) + (sp, dp, None), n * B, reps,
                kind_name(native.copy_kernel_kind(
                    d_elem, B, src.data_ptr(), dst.data_ptr()))
                + ("@base" if base is not None else "")),
        Variant("extra", lib.pa_device_copy,
                desc_args(d_extra, ssz) + (sp, dp, None), n * B, reps,
                kind_name(native.copy_kernel_kind(
                    d_extra, ssz, src.data_ptr(), dst.data_ptr()))),
    ]

    # (a) and (b) against an on-device permute of the B-byte elements
    want = src.view(n2, n1, n0, B).permute(2, 0, 1, 3).contiguous().view(-1)
    for v in vs[:2]:
        dst.fill_(0xAB)
        v.launch()
        torch.cuda.synchronize()
        if not torch.equal(dst, want):
            print(f"{label}: {v.name} MISMATCH vs torch permute")
            sys.exit(2)
    del want
    torch.cuda.empty_cache()

    for v in vs:  # warm-up
        v.launch()
    torch.cuda.synchronize()
    for _ in range(reps):
        for v in vs:
            v.timed()
    out = {v.name: v.report(label) for v in vs}
    del src, dst
    torch.cuda.empty_cache()
    return label, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None,
                    help="older build of libpencilhip.so for variant (b)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true",
                    help="128^3 only (tool self-test, counter runs)")
    a = ap.parse_args()
    assert a.reps >= 3
    lib = native.load()
    base = ctypes.CDLL(a.baseline_lib) if a.baseline_lib else None
    print(f"# comp_elem_bench reps={a.reps} "
          f"baseline_lib={'yes' if base else 'no'} "
          f"device={torch.cuda.get_device_name(0)}", flush=True)
    dims = (128,) * 3 if a.quick else (512,) * 3
    ok = True
    for ssz in (4, 8):
        label, r = run_shape(dims, ssz, lib, base, a.reps)
        # gate: the wide tile must beat the path it replaces by more than
        # the spread of either (its min above the other's max)
        win = r["wide"][1] > r["byteify"][2]
        ok &= win
        print(f"# gate {label}: wide min {r['wide'][1]:.1f} vs byteify max "
              f"{r['byteify'][2]:.1f} GB/s -> {'PASS' if win else 'FAIL'}")
        print(f"# wide/extra median ratio {label}: "
              f"{r['wide'][0] / r['extra'][0]:.3f}")
    print("# gate", "PASS" if ok else "FAIL")


if __name__ == "__main__":
    main()
