"""Launch the scaling tiles and the ordinary 8-byte tiles a few times each on
one dense (512, 512, 8) transpose, for a counters-only profiler run:

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR \
        --output-format csv -- python tools/scale_lds_probe.py
    python tools/scale_lds_probe.py --summarize DIR > profiles/scale_lds_conflict.txt

The summary sums both counters over the launches of each kernel.
"""

import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, NB, REPS = 512, 8, 3


def run():
    import torch
    from pencilarrays_amd import native
    desc = ((N, N, NB), (1, N, N * N), 0, (N, 1, N * N), 0)
    odd = ((N, N, NB), (1, N, N * N), 0, (N, 1, N * N), 1)  # off TILE_VS
    for code, isz, nscals in ((native.SCALAR_F64, 8, (1, 2, 3, 4)),
                              (native.SCALAR_F32, 4, (1, 2, 3, 4))):
        for nscal in nscals:
            nbytes = (N * N * NB + 1) * nscal * isz
            src = torch.randn(nbytes // 4, dtype=torch.float32,
                              device="cuda:0")
            dst = torch.empty_like(src)
            k = native.copy_kernel_kind_scale(desc, code, nscal,
                                              src.data_ptr(), dst.data_ptr())
            assert k.kind == native.KERNEL_SCALE_TILE, k
            for _ in range(REPS):
                native.device_copy_scale(desc, code, nscal, 0.5,
                                         src.data_ptr(), dst.data_ptr())
    src = torch.randn((N * N * NB + 1) * 2, dtype=torch.float32,
                      device="cuda:0")
    dst = torch.empty_like(src)
    for d, want in ((desc, native.KERNEL_TILE_VS), (odd, native.KERNEL_TILE)):
        k = native.copy_kernel_kind(d, 8, src.data_ptr(), dst.data_ptr())
        assert k.kind == want, k
        for _ in range(REPS):
            native.device_copy(d, 8, src.data_ptr(), dst.data_ptr())
    torch.cuda.synchronize()


def summarize(root):
    tot = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            if not fn.endswith("counter_collection.csv"):
                continue
            with open(os.path.join(dirpath, fn), newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row["Kernel_Name"]
                    if "tile" not in name:
                        continue
                    d = tot.setdefault(name, {"n": set()})
                    d["n"].add(row.get("Dispatch_Id"))
                    c = row["Counter_Name"]
                    d[c] = d.get(c, 0.0) + float(row["Counter_Value"])
    print("# rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE (counters "
          "only, no tracing) over tools/scale_lds_probe.py: a dense "
          f"({N}, {N}, {NB}) transpose, {REPS} launches per kernel, summed "
          "over the launches of each kernel")
    print(f"{'kernel':72s} {'launches':>8s} {'SQ_LDS_BANK_CONFLICT':>21s} "
          f"{'SQ_LDS_IDX_ACTIVE':>18s}")
    for name in sorted(tot):
        d = tot[name]
        print(f"{name[:72]:72s} {len(d['n']):8d} "
              f"{d.get('SQ_LDS_BANK_CONFLICT', 0):21.0f} "
              f"{d.get('SQ_LDS_IDX_ACTIVE', 0):18.0f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run()
