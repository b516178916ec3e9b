"""Times the symmetric eigensolver and its three callers on one device and writes one JSON line per case to profiles/eigh.jsonl
(the file is written, not appended to).  Five rounds after one warm-up, medians with min - max; a host route whose warm-up
takes more than 20 s is timed over two rounds, and the line says so ("rounds").
  eigh     Context.eigh on a CUDA tensor at n = 512, 2048, 8192, Gaussian symmetric and rank-n/3 Gram, with the sweeps used,
           against torch.linalg.eigh on the same device (a comparison line only: nothing in the library calls it) and, up to
           --host-max, numpy.linalg.eigh
  callers  quad_fit at 10^6 x 64 and 10^5 x 128, RbfInterp.fit at 2048 and 8192 supports (dim 3, cubic kernel, linear tail,
           8 right-hand sides), mvn_factor of a rank-deficient covariance at d = 2048: the device route against the host route
           in the same run, on the host threads the run saw (OMP_NUM_THREADS is recorded, never set)
Usage: python tools/bench_eigh.py [--cases eigh,callers] [--sizes 512,2048,8192] [--host-max 2048] [--out profiles/eigh.jsonl]
       python tools/bench_eigh.py --only-eigh 8192     one decomposition after a warm-up: the run a kernel trace wraps"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def matrix(kind, n):
    rng = np.random.default_rng(n)
    if kind == "gauss":
        g = rng.standard_normal((n, n))
        return 0.5 * (g + g.T)
    x = rng.standard_normal((n, n // 3))
    return x @ x.T


def timed(fn, sync, rounds=5, slow_s=None):
    t0 = time.perf_counter()
    fn()
    sync()
    if slow_s is not None and time.perf_counter() - t0 > slow_s:
        rounds = 2
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": rounds}


def eigh_cases(ctx, torch, emit, sizes, host_max):
    for n in sizes:
        for kind in ("gauss", "gram"):
            a = matrix(kind, n)
            t = torch.tensor(a, device="cuda")
            rec = {"case": "eigh", "kind": kind, "n": n, "device": timed(lambda: ctx.eigh(t), torch.cuda.synchronize)}
            rec["sweeps"], rec["route"] = ctx.last_eigh_info["sweeps"], ctx.last_eigh_route
            w, v = ctx.eigh(t)
            rec["residual_over_norm"] = float(torch.linalg.norm(t @ v - v * w) / torch.linalg.norm(t))
            rec["torch_linalg_eigh"] = timed(lambda: torch.linalg.eigh(t), torch.cuda.synchronize)
            if n <= host_max:
                rec["numpy_eigh"] = timed(lambda: np.linalg.eigh(a), lambda: None)
            emit(rec)


def caller_cases(ctx, torch, emit):
    from corrla_rs_amd import callers
    sync = torch.cuda.synchronize

    def both(rec, device, host):
        rec["device"] = timed(device, sync)
        rec["sweeps"] = ctx.last_eigh_info["sweeps"]
        rec["host"] = timed(host, sync, slow_s=20.0)
        rec["device_over_host"] = rec["device"]["median_ms"] / rec["host"]["median_ms"]
        emit(rec)

    for m, k in ((10 ** 6, 64), (10 ** 5, 128)):
        g = torch.Generator(device="cuda").manual_seed(k)
        x = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64) * 2.0 - 1.0
        y = (x[:, :8].sum(dim=1) + (x[:, 0] * x[:, 1]))[:, None].contiguous()
        p = k + k * (k + 1) // 2 + 1
        both({"case": "quad_fit", "m": m, "k": k, "p": p},
             lambda: callers.quad_fit(x, y, ctx=ctx, solve="device"), lambda: callers.quad_fit(x, y, ctx=ctx))
        del x, y
    for n_s in (2048, 8192):
        rng = np.random.default_rng(n_s)
        xs = torch.tensor(rng.uniform(-1.0, 1.0, (n_s, 3)), device="cuda")
        ys = torch.tensor(rng.standard_normal((n_s, 8)), device="cuda")
        both({"case": "rbf_fit", "n_s": n_s, "order": n_s + 4, "n_rhs": 8},
             lambda: callers.RbfInterp(3, 0.0, 3, 1, ctx=ctx, solver="eigh").fit(xs, ys),
             lambda: callers.RbfInterp(3, 0.0, 3, 1, ctx=ctx).fit(xs, ys))
    d = 2048
    z = np.random.default_rng(d).standard_normal((d // 4, d))
    z[:, 0] = z[:, 1] = 0.0
    z[0, 0] = z[0, 1] = 2.0      # an exactly zero Cholesky pivot on either route
    cov = z.T @ z
    cov = torch.tensor(np.tril(cov) + np.tril(cov, -1).T, device="cuda")
    both({"case": "mvn_factor", "d": d, "rank": d // 4},
         lambda: callers.mvn_factor(cov, device=True, ctx=ctx, eig="device"), lambda: callers.mvn_factor(cov, device=True, ctx=ctx))


def main():
    import torch
    import corrla_rs_amd as cr
    ctx = cr.Context(0)
    if "--only-eigh" in sys.argv:
        t = torch.tensor(matrix("gauss", int(arg("--only-eigh", "8192"))), device="cuda")
        ctx.eigh(t)
        torch.cuda.synchronize()
        ctx.eigh(t)
        torch.cuda.synchronize()
        print("sweeps", ctx.last_eigh_info["sweeps"])
        ctx.close()
        return
    cases = arg("--cases", "eigh,callers").split(",")
    sizes = [int(v) for v in arg("--sizes", "512,2048,8192").split(",")]
    out = arg("--out", os.path.join("profiles", "eigh.jsonl"))
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        def emit(rec):
            rec["omp_threads"] = os.environ.get("OMP_NUM_THREADS")
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if "eigh" in cases:
            eigh_cases(ctx, torch, emit, sizes, int(arg("--host-max", "2048")))
        if "callers" in cases:
            caller_cases(ctx, torch, emit)
    ctx.close()


if __name__ == "__main__":
    main()
