#!/usr/bin/env python3
"""PCA caller (PcaRsvd::new, pca_rsvd.rs:56-82) timing on device-resident data: n_samples x n_dim f64/f32,
rank k, the reference's hard-coded q = 20, p = min(n_dim, 10).  Prints one JSON line per config.
  --standardize [--out FILE]    the whole step with and without standardize=True (median of 10, min / max beside it), the A X
                                launch of the same operand, and at 16384^2 f32 a torch standardised copy followed by pca
  --variance-pass [--out FILE]  the variance pass alone, under a kernel trace (procedure: variance_pass_launches below and
                                tools/parse_variance_trace.py, which computes time, spread, GB/s on A and the ratio to A X)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

ctx = cr.Context(0)
SHAPES = ((100000, 1024, torch.float64, 16), (1000000, 256, torch.float32, 16), (16384, 16384, torch.float32, 32))


def _stats(fn, warmup=3, reps=10):
    """median / min / max wall time in ms of fn(), each run ended by a device synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "warmup": warmup, "reps": reps}


def _data(m, n, dt):
    x = torch.empty((m, n), dtype=dt, device="cuda")
    ctx.fill_normal(x, seed=11)
    x *= torch.linspace(3.0, 0.2, n, device="cuda", dtype=dt)
    x += torch.linspace(-2.0, 2.0, n, device="cuda", dtype=dt)
    return x


def standardize_steps(emit):
    """whole pca step, standardised against not (default centring), on the three shapes above; at 16384^2 f32 also the
    caller-side alternative: a standardised copy made with torch, then the plain pca"""
    for (m, n, dt, k) in SHAPES:
        x = _data(m, n, dt)
        l = k + min(n, 10)
        om = torch.randn((n, l), dtype=dt, device="cuda")
        ax_ms, _ = ctx.time_sketch(x, om, reps=10)     # the yardstick: one A X launch (l columns) on the same operand
        row = {"tool": "bench_pca", "what": "pca step", "m": m, "n": n, "dtype": str(dt).split(".")[-1], "k": k,
               "ax_launch_ms": round(ax_ms, 4), "plain": _stats(lambda: ctx.pca(x, k, seed=3)),
               "standardized": _stats(lambda: ctx.pca(x, k, seed=3, standardize=True))}
        if (m, n) == (16384, 16384):
            def torch_then_pca():
                xs = (x - x.mean(dim=0, keepdim=True)) / x.std(dim=0, keepdim=True)
                return ctx.pca(xs, k, seed=3)
            row["torch_standardized_copy_then_pca"] = _stats(torch_then_pca)
        emit(row)
        del x
        torch.cuda.empty_cache()


def variance_pass_launches(emit, reps=12):
    """The variance pass alone.  Its device time comes from a kernel trace, not from this process:
        rocprofv3 --kernel-trace -f csv -d DIR -- python tools/bench_pca.py --variance-pass --out OPERANDS.jsonl
        python tools/parse_variance_trace.py DIR OPERANDS.jsonl profiles/pca_standardize.jsonl
    Per operand this makes `reps` standardised calls without power iterations (so the colss_* / csr_colss launches of
    the trace come in the order of the rows emitted here, `reps` per operand) and emits the bytes of A the pass reads
    and the yardstick, one A X launch on the same operand: device time of ctx.time_sketch (hipEvents) for dense f32 /
    f64 operands at the l of the PCA step; for bf16 and CSR operands, which that hook does not take, the parser takes
    the product launches (gemm_bf16a / spmm kernels: A X and A^T X at l = 10, and the means at l = 1) from the trace."""
    def run(name, x, bytes_a, l=None):
        row = {"tool": "bench_pca", "what": "variance pass operand", "operand": name, "bytes_A": bytes_a, "launches": reps}
        for _ in range(reps):
            ctx.pca(x, 8, 0, 2, seed=3, standardize=True)
        torch.cuda.synchronize()
        if l is not None:
            om = torch.randn((x.shape[1], l), dtype=x.dtype, device="cuda")
            row["ax_launch_ms"], row["ax_l"] = round(ctx.time_sketch(x, om, reps=10)[0], 4), l
        emit(row)
    x = _data(16384, 16384, torch.float32)
    run("16384x16384 f32 row-major (down the rows)", x, x.numel() * 4, 42)
    run("16384x16384 f32 column-major (along the rows)", x.t(), x.numel() * 4, 42)
    xb = x.to(torch.bfloat16)
    run("16384x16384 bf16 row-major (down the rows)", xb, xb.numel() * 2)
    run("16384x16384 bf16 column-major (along the rows)", xb.t(), xb.numel() * 2)
    del x, xb
    torch.cuda.empty_cache()
    x = _data(1000000, 256, torch.float32)
    run("1000000x256 f32 row-major (down the rows)", x, x.numel() * 4, 26)
    del x
    x = _data(100000, 1024, torch.float64)
    run("100000x1024 f64 row-major (down the rows)", x, x.numel() * 8, 26)
    del x
    torch.cuda.empty_cache()
    # the CSR of profiles/sparse_rsvd.jsonl: 200000 x 20000 at density 0.001, f32.  Read per stored entry: the value, its
    # index and the index before it (the duplicate-run test); per row two row pointers
    m, n, nnz = 200000, 20000, 4000000
    g = torch.Generator(device="cuda").manual_seed(5)
    flat = torch.unique(torch.randint(0, m * n, (nnz,), device="cuda", generator=g))
    rows = torch.div(flat, n, rounding_mode="floor")
    crow = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    crow[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
    vals = torch.randn(flat.numel(), device="cuda", generator=g)
    a = torch.sparse_csr_tensor(crow, (flat - rows * n).to(torch.int32), vals, size=(m, n))
    run("csr 200000x20000 density 0.001 f32", a, int(flat.numel()) * 12 + (n + 1) * 8)


if "--standardize" in sys.argv or "--variance-pass" in sys.argv:
    out = open(sys.argv[sys.argv.index("--out") + 1], "a") if "--out" in sys.argv else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    (standardize_steps if "--standardize" in sys.argv else variance_pass_launches)(emit)
    sys.exit(0)

for (m, n, dt, k) in SHAPES:
    x = torch.empty((m, n), dtype=dt, device="cuda")
    ctx.fill_normal(x, seed=11)
    x *= torch.linspace(3.0, 0.2, n, device="cuda", dtype=dt)
    for center in ("copy", "fused"):
        for _ in range(2):
            out = ctx.pca(x, k, seed=3, center=center)
        torch.cuda.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            means, s, comps = ctx.pca(x, k, seed=3, center=center)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / reps * 1e3
        q, p = 20, min(n, 10)
        fl = cr.algorithmic_flops(m, n, k, q, p) + 2.0 * m * n  # + means and centring
        ev = (s.double() ** 2 / (m - 1)).ravel()[:3].tolist()
        print(json.dumps({"workload": f"PcaRsvd::new {m}x{n} {str(dt).split('.')[-1]} rank {k} (q=20, p={p})",
                          "center": center, "ms": round(ms, 3), "GFLOPs": round(fl / ms / 1e6, 1),
                          "explained_var_top3": [round(v, 4) for v in ev]}), flush=True)
    del x
    torch.cuda.empty_cache()
