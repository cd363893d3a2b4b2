#!/usr/bin/env python3
"""bench.py — transpose! effective GiB/s on MI355X (BASELINE.json metric).

A "step" is ONE x->y pencil transpose of the global grid (the hot path,
Transpositions.transpose!).  Default workload: 1024^3 Float64 x->y — the
configuration the BASELINE metric is quoted on — on N GPUs of one node with
the BASELINE grids (N=1: 1x1, 2: 2x1, 4: 2x2, 8: 2x4).

  python bench.py --gpus N --steps K --warmup W

For N>1 the driver launches this under torch.distributed.run with one rank
per GPU over RCCL; ranks read RANK/LOCAL_RANK/WORLD_SIZE from the env.

value = prod(size_global) * elem_size / t_step / 2^30 (whole-job effective
GiB/s; inputs resident in HBM when the timed region starts).  Also emitted:
`roofline` (dominant kernel, HIP-event timed over the same timed region,
algorithmic bytes vs the 8 TB/s HBM peak).

A plain run does only what the headline needs: set up, warm up, time the
steps, print the line.  `--full` adds everything that takes runs of its own:
the checksum self-verification (`verify`), the per-stage HIP-event step
(`stage_ms`), the identity-layout variant (`variant_identity`, N=1) and
`cpu_baseline` (the C oracle restatement timed on the host cores, rank 0 at
N=1 only).  `--dump-outputs DIR` writes what the last timed step computed as
DIR/<name>.npy (a fixed seeded sample when the output is large); the inputs
are seeded, so two builds can be compared output for output.
"""

import argparse
import json
import math
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# the host driver only supports dmabuf IPC; without this, RCCL across
# processes fails with hipIpcGetMemHandle errors (normally exported by the
# environment — kept here as insurance for the multi-process run)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# surface RCCL warnings/errors in stderr for the unattended N>1 run
# (default VERSION level prints only the banner)
os.environ.setdefault("NCCL_DEBUG", "WARN")

import torch  # noqa: E402

from pencilarrays_amd import Pencil, PencilArray, Topology, Transposition  # noqa: E402

DEFAULT_GRIDS = {1: (1, 1), 2: (2, 1), 4: (2, 2), 8: (2, 4)}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[1024, 1024, 1024])
    ap.add_argument("--grid", type=int, nargs=2, default=None,
                    help="process grid P1 P2 (default: BASELINE grids)")
    ap.add_argument("--permuted", action="store_true", default=True,
                    help="output pencil memory-permuted (1,2,0) — the "
                         "PencilFFTs layout (test/transpose.jl:29-30). "
                         "DEFAULT: this is the realistic workload; at grid "
                         "1x1 an identity-layout x->y collapses to a plain "
                         "device copy")
    ap.add_argument("--identity", dest="permuted", action="store_false",
                    help="identity memory layout variant (at 1x1 this is a "
                         "straight copy; reported as variant_identity in "
                         "the default run)")
    ap.add_argument("--double", action="store_true",
                    help="config-4 variant: x->y->z chained double "
                         "transpose (PencilFFTs pattern), deferred waits")
    ap.add_argument("--dtype", default="float64",
                    choices=["float64", "complex64"])
    ap.add_argument("--chunks", type=int, default=1,
                    help="split the RCCL exchange into N chunks and unpack "
                         "each as it lands (the reference's Waitany overlap; "
                         "1 = single grouped exchange)")
    ap.add_argument("--full", action="store_true",
                    help="also run the extra legs: checksum verification, "
                         "per-stage timing step, identity-layout variant "
                         "and CPU baseline (N=1)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as "
                         "DIR/<name>.npy (seeded sample if large)")
    return ap.parse_args()


def cpu_baseline(sample=(512, 512, 512), reps=8):
    """Time the line-faithful C oracle (the reference algorithm, OpenMP over
    this box's host cores) on a bounded sample of the same workload: world=1
    x->y, Float64 — kind 'port' (restatement), reported as context."""
    exe = os.path.join(REPO, "oracle", "oracle_bench")
    if not os.path.exists(exe):
        try:
            subprocess.run(["make", "-C", os.path.join(REPO, "oracle"),
                            "oracle_bench"], check=True, capture_output=True)
        except Exception:
            return None
    try:
        out = subprocess.run(
            [exe, str(sample[0]), str(sample[1]), str(sample[2]), "1", "1",
             str(reps)],
            capture_output=True, text=True, timeout=600, check=True)
        r = json.loads(out.stdout.strip().splitlines()[-1])
        return {
            "value": round(r["gib_per_s"], 3),
            "unit": "GiB/s",
            "cores": r["threads"],
            "kind": "port",
            "sample": f"{sample[0]}^3 Float64 x->y world=1, best of {reps} "
                      f"(the reference algorithm incl. its staged self-copy)",
        }
    except Exception:
        return None


# --dump-outputs budget: 32 MiB per run in all, split over ranks and arrays
DUMP_BUDGET_BYTES = 32 << 20
DUMP_SEED = 0x5EED


def dump_output(dirname, name, ten, budget_bytes):
    """Write `ten` (1-D device tensor) as dirname/name.npy in float32/float64
    (complex as interleaved re,im).  Outputs above the budget are sampled at
    a fixed seeded set of element indices, identical from run to run."""
    import numpy as np
    n = ten.numel()
    keep = max(1, budget_bytes // ten.element_size())
    if n > keep:
        idx = np.sort(np.random.default_rng(DUMP_SEED).integers(
            0, n, size=keep, dtype=np.int64))
        ten = ten.index_select(0, torch.from_numpy(idx).to(ten.device))
    if ten.is_complex():
        ten = torch.view_as_real(ten)
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, name + ".npy"), ten.cpu().numpy())


def main():
    args = parse_args()
    if args.chunks > 1:
        os.environ["PENCILHIP_EXCHANGE_CHUNKS"] = str(args.chunks)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(world, args.gpus)

    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # Control plane on GLOO: barriers/allreduce/uid-exchange only.  The
        # engine's own RCCL communicators are then the ONLY NCCL-family
        # comms per device (interleaving a torch-NCCL comm with the engine's
        # grouped send/recv is a known deadlock hazard).
        dist.init_process_group("gloo", rank=rank, world_size=world)

    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    grid = tuple(args.grid) if args.grid else DEFAULT_GRIDS.get(
        n_gpus, (2, n_gpus // 2))
    assert math.prod(grid) == n_gpus, f"grid {grid} != {n_gpus} ranks"

    dims = tuple(args.size)
    tdt = {"float64": torch.float64, "complex64": torch.complex64}[args.dtype]
    esz = torch.tensor([], dtype=tdt).element_size()

    topo = Topology(grid)
    Pi = Pencil(topo, dims, (1, 2))

    gen = torch.Generator(device=device).manual_seed(0xC0FFEE + rank)
    n_in = Pi.length_local(rank)
    src_t = torch.empty(n_in, dtype=tdt, device=device)
    # fill in <=2^30-element chunks (some torch fill kernels reject >2^31
    # element launches; our own kernels are 64-bit-indexed throughout)
    CH = 1 << 30
    for off in range(0, n_in, CH):
        sl = src_t[off:off + CH]
        sl.copy_(torch.randn(sl.numel(), generator=gen, dtype=tdt,
                             device=device))
    src = PencilArray(Pi, rank, src_t)

    def measure(permuted, dump_dir=None):
        """One measurement (setup + warmup + timed region; with --full also
        verify + stage times) of the x->y (or x->y->z) transpose; returns a
        dict."""
        po_perm = (1, 2, 0) if (permuted or args.double) else None
        Po = Pencil(topo, dims, (0, 2), permute=po_perm)
        Pz = (Pencil(topo, dims, (0, 1), permute=(2, 1, 0))
              if args.double else None)
        dst = PencilArray(Po, rank, torch.empty(
            Po.length_local(rank), dtype=tdt, device=device))

        t = Transposition(dst, src)
        t.execute()  # builds native plan, binds staging, inits RCCL comms
        t2 = dstz = None
        if args.double:
            dstz = PencilArray(Pz, rank, torch.empty(
                Pz.length_local(rank), dtype=tdt, device=device))
            t2 = Transposition(dstz, dst)
            t2.execute()
        torch.cuda.synchronize()

        stream = torch.cuda.current_stream()

        def step(sync=False):
            # deferred waits (waitall=false pattern): hops enqueue, the
            # stream orders them
            t._native.execute(src.data, dst.data, sync=False)
            if t2 is not None:
                t2._native.execute(dst.data, dstz.data, sync=False)
            if sync:
                torch.cuda.synchronize()

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
            torch.cuda.synchronize()

        # HIP events around the timed region on the launch stream: per-step
        # kernel-side duration for the roofline (single-kernel steps at N=1).
        ev_a = torch.cuda.Event(enable_timing=True)
        ev_b = torch.cuda.Event(enable_timing=True)
        ev_a.record(stream)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        ev_b.record(stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if dist:
            dist.barrier()
            torch.cuda.synchronize()
        elapsed = t1 - t0
        gpu_ms = ev_a.elapsed_time(ev_b)

        if dist:
            tmax = torch.tensor([elapsed])  # CPU tensor: gloo
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())

        # what the last timed step left in the output arrays
        if dump_dir:
            outs = [("dst", dst.data)]
            if t2 is not None:
                outs.append(("dstz", dstz.data))
            for name, ten in outs:
                if world > 1:
                    name = f"{name}_rank{rank}"
                dump_output(dump_dir, name, ten,
                            DUMP_BUDGET_BYTES // (world * len(outs)))

        if not args.full:
            return {
                "elapsed": elapsed,
                "gpu_ms": gpu_ms,
                "verify": None,
                "stage_ms": None,
                "permuted": permuted,
                "nproc_sub": t._native.native.nproc_sub,
            }

        # Per-stage HIP-event times (TimerOutputs analogue): one extra
        # untimed step with timing events enabled, AFTER the timed region.
        stage_ms = None
        try:
            t._native.native.enable_timing(True)
            if t2 is not None:
                t2._native.native.enable_timing(True)
            step(sync=True)

            def fmt(native):
                return {k: (round(v, 4) if v is not None else None)
                        for k, v in native.stage_times().items()}
            stage_ms = fmt(t._native.native)
            t._native.native.enable_timing(False)
            if t2 is not None:
                stage_ms = {"hop_xy": stage_ms,
                            "hop_yz": fmt(t2._native.native)}
                t2._native.native.enable_timing(False)
        except Exception as exc:  # never fail the bench over telemetry
            stage_ms = {"error": str(exc)}

        # Self-verification (outside the timed region): the transpose is
        # pure data movement, so the wrap-around sum of the int64 bit
        # patterns is conserved exactly, whole-job, independent of order
        # and distribution.
        def bit_checksum(ten):
            v = ten.view(torch.int64) if ten.dtype != torch.int64 else ten
            s = v.sum().cpu()  # int64 wrap-around == modular, exact
            if dist:
                dist.all_reduce(s, op=dist.ReduceOp.SUM)
            return int(s.item())

        cks_src = bit_checksum(src.data)
        cks_dst = bit_checksum(dstz.data if t2 is not None else dst.data)
        return {
            "elapsed": elapsed,
            "gpu_ms": gpu_ms,
            "verify": "ok" if cks_src == cks_dst else "FAIL",
            "stage_ms": stage_ms,
            "permuted": permuted,
            # real subgroup size of the transposed dimension (the exchange
            # group), from the plan — not assumed from the grid shape
            "nproc_sub": t._native.native.nproc_sub,
        }

    m = measure(args.permuted, dump_dir=args.dump_outputs)
    # the identity-layout variant (at 1x1: a straight device copy) measured
    # alongside the headline when it differs from it (N=1 default runs)
    variant = None
    if args.full and n_gpus == 1 and args.permuted and not args.double:
        mi = measure(False)
        variant = {
            "workload": "identity memory layout (collapses to device copy)",
            "value": round(math.prod(dims) * esz /
                           (mi["elapsed"] / args.steps) / 2**30, 2),
            "ms_per_step": round(mi["elapsed"] / args.steps * 1e3, 4),
            "verify": mi["verify"],
        }

    if dist:
        dist.barrier()
        dist.destroy_process_group()

    elapsed, gpu_ms, verify = m["elapsed"], m["gpu_ms"], m["verify"]
    ms_per_step = elapsed / args.steps * 1e3
    global_bytes = math.prod(dims) * esz
    nhops = 2 if args.double else 1
    gib_s = nhops * global_bytes / (elapsed / args.steps) / 2**30

    if rank != 0:
        return

    # Roofline of the dominant kernel.  At N=1 the whole step is the fused
    # local copy: algorithmic HBM traffic = 2 * elem_size per global element
    # (read + write; the reference's staged path moves 4x).  At
    # N>1 the dominant resource is the xGMI link: each of the P_sub-1 peers
    # rides its own point-to-point link, so per-link bytes per step =
    # local_bytes/P_sub each direction (the remote fraction split evenly).
    P_sub = m["nproc_sub"]
    hops = nhops
    if n_gpus == 1:
        kernel_ms = gpu_ms / args.steps / hops
        algo_bytes = 2 * global_bytes  # per launch == per hop at N=1
        # traffic: measured with rocprofv3 PMC on this exact kernel+workload
        # (profiles/r01_pmc_traffic.md): FETCH_SIZE*2 (gfx950 wide-coalesced
        # correction) + WRITE_SIZE == algorithmic bytes, no re-reads.
        measured_traffic = (algo_bytes
                            if tuple(dims) == (1024, 1024, 1024) else None)
        kname = ("k_transpose_tile (fused local permuted copy)"
                 if args.permuted or args.double
                 else "k_copy_1d (fused local copy, identity layout)")
        roofline = {
            "bound": "hbm",
            "achieved": round(algo_bytes / (kernel_ms * 1e-3) / 1e9, 1),
            "peak": 8000.0,
            "unit": "GB/s",
            "frac": round(algo_bytes / (kernel_ms * 1e-3) / 8e12, 4),
            "traffic": measured_traffic,
            "traffic_source": ("rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE, "
                               "profiles/r2_kernel_stats.md"
                               if measured_traffic else None),
            "kernel": kname,
        }
    else:
        local_bytes = global_bytes // n_gpus
        remote_frac = (P_sub - 1) / P_sub
        link_bytes = local_bytes * remote_frac / max(P_sub - 1, 1)
        roofline = {
            "bound": "xgmi",
            "achieved": round(link_bytes / (elapsed / args.steps) / 1e9, 1),
            "peak": 153.0,
            "unit": "GB/s",
            "frac": round(link_bytes / (elapsed / args.steps) / 153e9, 4),
            "traffic": None,
            "kernel": "per-link xGMI send (grouped ncclSend/Recv)",
        }

    cb = None
    if args.full and n_gpus == 1 and not args.no_cpu_baseline:
        cb = cpu_baseline()

    sz = "x".join(map(str, dims))
    result = {
        "metric": "transpose! effective GiB/s (1024^3 Float64 x->y pencil)",
        "value": round(gib_s, 2),
        "unit": "GiB/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "verify": verify,
        "dtype": "f64" if args.dtype == "float64" else "c64",
        "data": "synthetic",
        "config": {
            "workload": f"{sz} {args.dtype} "
                        + ("x->y->z double transpose (PencilFFTs pattern, "
                           "deferred waits)" if args.double else
                           "x->y pencil transpose"
                           + (" (memory-permuted output, PencilFFTs layout)"
                              if args.permuted else "")),
            "grid": f"{grid[0]}x{grid[1]}",
            "exchange": "rccl" if n_gpus > 1 else "none (local path)",
        },
        "roofline": roofline,
        "cpu_baseline": cb,
        "stage_ms": m["stage_ms"],
    }
    if variant is not None:
        result["variant_identity"] = variant
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
