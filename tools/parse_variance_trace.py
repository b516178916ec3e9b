#!/usr/bin/env python3
"""Kernel trace of `tools/bench_pca.py --variance-pass` -> one JSON line per operand, appended to the profile file:
median / min / max device time of the variance-pass launch (colss_down / colss_along / csr_colss kernel; the first
launch of every operand is left out as warm-up), GB/s on the bytes of A it reads, and the ratio to one A X launch on the
same operand (ax_launch_ms of the operand row where the tool measured it with hipEvents, else the median of the
operand's product launches in the trace, named in "ax_from").

    python tools/parse_variance_trace.py TRACE_DIR OPERANDS.jsonl OUT.jsonl"""
import csv
import glob
import json
import sys

trace_dir, operands, out = sys.argv[1:4]
passes, products = [], []
for f in glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        rec = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name)
        if "colss_down" in name or "colss_along" in name or "csr_colss_kernel" in name:
            passes.append(rec)
        elif "gemm_bf16a_kernel" in name or "spmm" in name:
            products.append(rec)
passes.sort()
ops = [json.loads(line) for line in open(operands)]
assert len(passes) == sum(o["launches"] for o in ops), (len(passes), "variance-pass launches in the trace")


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


i = 0
with open(out, "a") as fo:
    for o in ops:
        grp = passes[i:i + o["launches"]]
        i += o["launches"]
        med, lo, hi = stats([(e - s) / 1e6 for s, e, _ in grp[1:]])
        rec = {"tool": "bench_pca --variance-pass + parse_variance_trace", "operand": o["operand"],
               "kernel": grp[0][2].split("<")[0].split("::")[-1], "launches_timed": len(grp) - 1, "median_ms": round(med, 4),
               "min_ms": round(lo, 4), "max_ms": round(hi, 4), "bytes_A": o["bytes_A"], "GBps_on_A": round(o["bytes_A"] / med / 1e6, 1)}
        if "ax_launch_ms" in o:
            rec["ax_launch_ms"], rec["ax_l"], rec["ax_from"] = o["ax_launch_ms"], o["ax_l"], "time_sketch (hipEvents, mean of 10)"
        else:
            t0, t1 = grp[0][0], grp[-1][1]
            mine = [(e - s) / 1e6 for s, e, n in products if t0 <= s <= t1 + 50_000_000]
            if mine:
                pm, plo, phi = stats(mine)
                rec["ax_launch_ms"], rec["ax_from"] = round(pm, 4), "median of %d product launches of the trace (min %.4f, max %.4f)" % (len(mine), plo, phi)
        if "ax_launch_ms" in rec:
            rec["ratio_to_ax"] = round(med / rec["ax_launch_ms"], 3)
        print(json.dumps(rec))
        fo.write(json.dumps(rec) + "\n")
