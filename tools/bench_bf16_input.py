#!/usr/bin/env python3
"""Dense bf16 input against the exact f32 path on the same matrix widened to f32: the whole random_svd step and one
A X launch, per shape.  The two are timed ALTERNATELY in one process (rounds of f32, bf16, f32, bf16, ...), after a
warm-up of every shape and path, so clock ramp and neighbours on the machine hit both alike; the spread of the f32
rounds is recorded next to the ratio it qualifies.
   python tools/bench_bf16_input.py [C2] [C4shard] [fat] [--out profiles/bf16_input.jsonl]   -> one JSON line per shape"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

# name: (m, n, k, q, p)
CFG = {"C2": (16384, 16384, 128, 2, 10), "C4shard": (1_250_000, 512, 64, 2, 10), "fat": (4096, 262144, 128, 2, 10)}
ROUNDS, REPS, WARMUP = 5, 4, 3


def _step_ms(ctx, a, k, q, p):
    """mean wall time of REPS back-to-back calls, ended by a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        ctx.rsvd(a, k, q, p, seed=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


def _product_ms(ctx, a, x, n_launch=6):
    """device time of one A X launch sequence: hipEvents around the sketch product of a call, averaged over calls"""
    del x
    ms = 0.0
    for _ in range(n_launch):
        ctx.rsvd(a, 8, 0, 130, seed=2)          # q = 0: sketch, thin-Q, projection; l = 138 columns
        ms += ctx.timings()["sketch_kernel_ms"]
    return ms / n_launch


def main():
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    names = [a for a in args if a in CFG] or list(CFG)
    ctx = cr.Context(0)
    ctx.set_phase_timings(False)
    lines = []
    for name in names:
        m, n, k, q, p = CFG[name]
        a32 = torch.empty((m, n), dtype=torch.float32, device="cuda")
        ctx.fill_normal(a32, seed=20241008)
        a16 = a32.to(torch.bfloat16)
        a32.copy_(a16)                           # the same values on both sides: the bf16 matrix widened to f32
        ops = {"f32": a32, "bf16": a16}
        for _ in range(WARMUP):
            for a in ops.values():
                out = ctx.rsvd(a, k, q, p, seed=1)
        n_bf16 = ctx.timings()["n_bf16_products"]
        s16 = out[1].double().ravel()
        s32 = ctx.rsvd(a32, k, q, p, seed=1)[1].double().ravel()
        step = {"f32": [], "bf16": []}
        prod = {"f32": [], "bf16": []}
        for _ in range(ROUNDS):
            for key, a in ops.items():
                step[key].append(_step_ms(ctx, a, k, q, p))
        l_prod = min(8 + 130, min(m, n))
        for _ in range(ROUNDS):
            for key, a in ops.items():
                prod[key].append(_product_ms(ctx, a, None))
        med = {key: statistics.median(v) for key, v in step.items()}
        pmed = {key: statistics.median(v) for key, v in prod.items()}
        rec = {"shape": name, "m": m, "n": n, "k": k, "q": q, "p": p, "rounds": ROUNDS, "reps_per_round": REPS,
               "step_ms_f32": [round(v, 3) for v in step["f32"]], "step_ms_bf16": [round(v, 3) for v in step["bf16"]],
               "step_ms_f32_median": round(med["f32"], 3), "step_ms_bf16_median": round(med["bf16"], 3),
               "step_ratio_bf16_over_f32": round(med["bf16"] / med["f32"], 4),
               "step_f32_spread": round((max(step["f32"]) - min(step["f32"])) / med["f32"], 4),
               "product_columns": l_prod,
               "product_ms_f32": round(pmed["f32"], 4), "product_ms_bf16": round(pmed["bf16"], 4),
               "product_ratio_bf16_over_f32": round(pmed["bf16"] / pmed["f32"], 4),
               "product_A_GBps_f32": round(m * n * 4 / pmed["f32"] / 1e6, 0),
               "product_A_GBps_bf16": round(m * n * 2 / pmed["bf16"] / 1e6, 0),
               "n_bf16_products": n_bf16,
               "max_dS_over_s1_bf16_vs_f32": float((s16 - s32).abs().max() / s32[0])}
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del a32, a16, ops
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
