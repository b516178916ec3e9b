"""Sparse rsvd measurements (one GPU): the whole rsvd step on CSR input and its two tall products, against the dense
path on the same matrix densified where that fits on the device.

  python tools/bench_sparse.py [--out profiles/sparse_rsvd.jsonl] [--dtypes f32,f64] [--no-dense] [--no-large]

Method: k = 32, q = 2, p = 10, a seeded uniform-random pattern with Gaussian values built on the
device, 3 warm-up calls, median of 10, device time from the hipEvents the library records on its own stream
(Context.timings()).  The products are the ones inside the step: `sketch_kernel_ms` brackets Y = A Omega (A . X) and, with
phase timings on, `project_ms` brackets B^T = A^T Q (A^T . Y); for the sparse path both include the l-wide transposition
of the skinny operand.  Bytes per product: nnz (sizeof(T) + 4) + (rows + cols) L sizeof(T).

The dense kernels are selected by CORRLA_RSVD_LIB when it is set (another build of the library, e.g. the parent
commit's); otherwise the dense figures come from this build, whose dense kernels and plans are the parent's.
One JSON line per (shape, density, dtype)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, Q, P = 32, 2, 10
WARMUP, REPS = 3, 10


def make_csr(torch, m, n, nnz, dtype, seed):
    """uniform-random pattern (duplicates merged), N(0,1) values, as a CUDA torch.sparse_csr tensor"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat = torch.randint(0, m * n, (nnz,), device="cuda", generator=g, dtype=torch.int64)
    flat = torch.unique(flat)  # sorted
    rows = torch.div(flat, n, rounding_mode="floor")
    cols = (flat - rows * n).to(torch.int32)
    del flat
    crow = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
    del rows
    vals = torch.randn(cols.numel(), device="cuda", generator=g, dtype=dtype)
    return torch.sparse_csr_tensor(crow, cols, vals, size=(m, n))


def measure(ctx, a, reps=REPS, warmup=WARMUP):
    tot, ax, atx = [], [], []
    for i in range(warmup + reps):
        ctx.rsvd(a, K, Q, P, seed=17)
        if i >= warmup:
            t = ctx.timings()
            tot.append(t["total_ms"])
            ax.append(t["sketch_kernel_ms"])
            atx.append(t["project_ms"])
    med = statistics.median
    return med(tot), med(ax), med(atx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_rsvd.jsonl"))
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    import torch
    import corrla_rs_amd as cr
    ctx = cr.Context(0)
    ctx.set_phase_timings(True)
    cases = [(200_000, 20_000, d) for d in (0.001, 0.01, 0.05)]
    if not args.no_large:
        cases.append((4_000_000, 100_000, 1e-4))
    free = torch.cuda.mem_get_info()[0]
    lines = []
    for name in args.dtypes.split(","):
        dt = torch.float32 if name == "f32" else torch.float64
        esz = 4 if name == "f32" else 8
        for m, n, dens in cases:
            a = make_csr(torch, m, n, int(round(dens * m * n)), dt, seed=m + n)
            nnz = a.values().numel()
            l = min(K + P, n)
            tot, ax, atx = measure(ctx, a)
            nbytes = nnz * (esz + 4) + (m + n) * l * esz
            rec = {"tool": "bench_sparse", "m": m, "n": n, "density": dens, "nnz": nnz, "dtype": name, "k": K, "q": Q, "p": P,
                   "l": l, "warmup": WARMUP, "reps": REPS, "sparse_step_ms": round(tot, 4), "sparse_ax_ms": round(ax, 4),
                   "sparse_atx_ms": round(atx, 4), "product_bytes": nbytes,
                   "sparse_ax_gbps": round(nbytes / ax / 1e6, 1), "sparse_atx_gbps": round(nbytes / atx / 1e6, 1)}
            dense_bytes = m * n * esz
            if not args.no_dense and dense_bytes * 1.3 < free:
                d = a.to_dense()
                del a
                dtot, dax, datx = measure(ctx, d)
                del d
                rec.update({"dense_step_ms": round(dtot, 4), "dense_ax_ms": round(dax, 4), "dense_atx_ms": round(datx, 4),
                            "step_ratio_sparse_over_dense": round(tot / dtot, 4), "ax_ratio_sparse_over_dense": round(ax / dax, 4),
                            "atx_ratio_sparse_over_dense": round(atx / datx, 4),
                            "dense_lib": os.environ.get("CORRLA_RSVD_LIB", "this build")})
            else:
                del a
                rec["dense"] = "not measured" if args.no_dense else "does not fit on the device"
            torch.cuda.empty_cache()
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
