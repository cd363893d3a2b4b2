# Time permuted transposes of 1- and 2-byte elements standalone via
# pa_device_copy + HIP events, variants interleaved in one process:
#   (a) packed    the packed 1-/2-byte LDS tile (aligned buffers)
#   (b) scalar    the scalar LDS tile of this tree, forced by base pointers
#                 offset by one element (no knob needed)
#   (c) byteify   the byte-ify path of an older build of the library, loaded
#                 side by side through --baseline-lib PATH (esz 2 only: that
#                 path cannot run 1-byte transposes, its byte-ified 1-byte
#                 descriptor is the descriptor itself)
#   (d) f32       float32 on the same dims in this tree (4-byte scalar
#                 tile): the bytes/s yardstick
# Shapes: the N=1 headline x->y with output permutation (1,2,0) on 1024^3 and
# 2048x1024x1024, and the 8-GPU 2x4 per-peer pack / unpack descriptors of
# the 1024^3 plan.  Reported: MEDIAN GB/s (2*esz bytes per element) with
# min..max over the timed reps of that variant.
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pencilarrays_amd import Pencil, Topology, build_plan, native  # noqa: E402

I64 = ctypes.c_int64
T_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.float32}


def desc_args(desc, esz, src_t, dst_t):
    nd = len(desc.dims)
    return (nd, (I64 * nd)(*desc.dims), (I64 * nd)(*desc.sstrides),
            I64(desc.soffset), (I64 * nd)(*desc.dstrides), I64(desc.doffset),
            I64(esz), ctypes.c_void_p(src_t.data_ptr()),
            ctypes.c_void_p(dst_t.data_ptr()), None)


class Variant:
    def __init__(self, name, lib, desc, esz, src_t, dst_t, reps, kind):
        self.name, self.lib, self.reps, self.kind = name, lib, reps, kind
        self.args = desc_args(desc, esz, src_t, dst_t)
        self.gb = desc.nelem * esz * 2 / 1e9
        self.ms = []

    def launch(self):
        st = self.lib.pa_device_copy(*self.args)
        if st != 0:
            raise RuntimeError(f"{self.name}: pa_device_copy failed")

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
        print(f"{label:34s} {self.name:8s} {self.kind:10s} "
              f"median {med:8.1f} GB/s  min {gbs[0]:8.1f}  max {gbs[-1]:8.1f}"
              f"  ({statistics.median(self.ms):.3f} ms, n={len(self.ms)})",
              flush=True)
        return med, gbs[0], gbs[-1]


def kind_name(desc, esz, s, d):
    k = native.copy_kernel_kind(desc, esz, s.data_ptr(), d.data_ptr())
    return f"{native.KERNEL_NAMES[k.kind]}/w{k.word_bytes}"


def run_shape(label, desc, src_n, dst_n, esz, lib, base, reps, base_reps,
              check=None):
    dev = "cuda:0"
    src = torch.empty(src_n + 1, dtype=T_BITS[esz], device=dev)
    src.view(torch.uint8).random_(0, 256)
    dst = torch.empty(dst_n + 1, dtype=T_BITS[esz], device=dev)
    # (b) reads/writes the SAME data one element further on: src[1:], dst[1:]
    src_b = torch.empty_like(src)
    src_b[1:] = src[:-1]
    f_src = torch.empty(src_n, dtype=torch.float32, device=dev).normal_()
    f_dst = torch.empty(dst_n, dtype=torch.float32, device=dev)

    vs = [Variant("packed", lib, desc, esz, src, dst, reps,
                  kind_name(desc, esz, src, dst)),
          Variant("scalar", lib, desc, esz, src_b[1:], dst[1:], reps,
                  kind_name(desc, esz, src_b[1:], dst[1:])),
          Variant("f32", lib, desc, 4, f_src, f_dst, reps,
                  kind_name(desc, 4, f_src, f_dst))]
    if base is not None and esz == 2:
        vs.append(Variant("byteify", base, desc, esz, src, dst, base_reps,
                          "byte-ify"))

    if check is not None:  # packed and scalar outputs vs an on-device permute
        want = check(src[:src_n])
        for v, out in ((vs[0], dst[:dst_n]), (vs[1], dst[1:dst_n + 1])):
            dst.view(torch.uint8).fill_(0xAB)
            v.launch()
            torch.cuda.synchronize()
            if not torch.equal(out, want):
                print(f"{label}: {v.name} MISMATCH vs torch permute")
                sys.exit(2)
        del want
    for v in vs:  # warm-up
        v.launch()
    torch.cuda.synchronize()
    for rep in range(max(v.reps for v in vs)):
        for v in vs:
            if rep < v.reps:
                v.timed()
    out = {v.name: v.report(f"{label} esz{esz}") for v in vs}
    del src, dst, src_b, f_src, f_dst
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None,
                    help="older build of libpencilhip.so for variant (c)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--baseline-reps", type=int, default=3,
                    help="timed reps of (c): one launch of it takes long")
    ap.add_argument("--quick", action="store_true",
                    help="256^3 shapes only (tool self-test)")
    a = ap.parse_args()
    assert a.reps >= 10
    lib = native.load()
    base = ctypes.CDLL(a.baseline_lib) if a.baseline_lib else None
    print(f"# small_elem_bench reps={a.reps} baseline_reps={a.baseline_reps} "
          f"baseline_lib={'yes' if base else 'no'} "
          f"device={torch.cuda.get_device_name(0)}", flush=True)

    topo1 = Topology((1, 1))
    shapes = [(256, 256, 256)] if a.quick else \
        [(1024, 1024, 1024), (2048, 1024, 1024)]
    results = {}
    for dims in shapes:
        Pi = Pencil(topo1, dims, (1, 2))
        Po = Pencil(topo1, dims, (0, 2), permute=(1, 2, 0))
        p = build_plan(Pi, Po, 0)
        n = Pi.length_local(0)
        n0, n1, n2 = dims

        def check(s):
            return s.view(n2, n1, n0).permute(2, 0, 1).contiguous().view(-1)

        for esz in (2, 1):
            label = "N=1 perm " + "x".join(map(str, dims))
            results[(label, esz)] = run_shape(
                label, p.local, n, n, esz, lib, base, a.reps,
                a.baseline_reps, check)

    gdims = (256,) * 3 if a.quick else (1024,) * 3
    topo = Topology((2, 4))
    Pi = Pencil(topo, gdims, (1, 2))
    Po = Pencil(topo, gdims, (0, 2), permute=(1, 2, 0))
    p = build_plan(Pi, Po, 0)
    blk = next(b for b in p.peers
               if b.pack is not None and b.unpack is not None)
    for esz in (2, 1):
        run_shape(f"8gpu 2x4 pack k={blk.peer_k}", blk.pack,
                  Pi.length_local(0), max(p.send_nelem_total, 1), esz, lib,
                  base, a.reps, a.baseline_reps)
        run_shape(f"8gpu 2x4 unpack k={blk.peer_k}", blk.unpack,
                  max(p.recv_nelem_total, 1), Po.length_local(0), esz, lib,
                  base, a.reps, a.baseline_reps)

    # gate on the headline shapes: packed must beat scalar and byte-ify by
    # more than the spread seen in this run (its min above their max)
    ok = True
    for (label, esz), r in results.items():
        for other in ("scalar", "byteify"):
            if other in r:
                win = r["packed"][1] > r[other][2]
                ok &= win
                print(f"# gate {label} esz{esz}: packed min "
                      f"{r['packed'][1]:.1f} vs {other} max "
                      f"{r[other][2]:.1f} GB/s -> "
                      f"{'PASS' if win else 'FAIL'}")
        print(f"# packed/f32 median ratio {label} esz{esz}: "
              f"{r['packed'][0] / r['f32'][0]:.3f}")
    print("# gate", "PASS" if ok else "FAIL")


if __name__ == "__main__":
    main()
