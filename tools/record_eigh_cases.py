"""Runs the numpy restatement of the symmetric eigensolver (tests/eigh_reference.py) once on every case of the GPU test
(GPU_CALLS of tests/test_eigh_plan.py) and stores, per case, the sweeps and the error ratios of the restatement and of LAPACK
in tests/golden/eigh_cases.json.  tests/test_gpu_eigh.py takes its working bounds from that file (4 x the recorded value,
never above the fixed cap), so the file is regenerated only when the algorithm, a family or the list of cases changes.
Usage: python tools/record_eigh_cases.py [--jobs N]"""
import json
import multiprocessing
import os
import sys

# one BLAS thread per worker: the order of BLAS's sums can follow its thread count, and the eigenvalue distances recorded here
# are a few roundings of |A|.  The committed file was recorded this way, against the eigenvalues of numpy.linalg.eigh
# (numpy.linalg.eigvalsh takes another LAPACK path and differs from it by a few ulps, four times the recorded distance at
# rbf-129).
for _var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_var] = "1"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import eigh_reference as R  # noqa: E402
from tests.test_eigh_plan import GPU_CALLS  # noqa: E402


def record(case):
    name, n = case
    a = R.family(name, n)
    w, v, sweeps = R.restatement(a)
    wl, vl = np.linalg.eigh(a)
    mine, lapack = R.ratios(a, w, v, wl), R.ratios(a, wl, vl, wl)
    return R.case_id(name, n), {"sweeps": int(sweeps), "residual": mine["residual"], "orth": mine["orth"], "eig": mine["eig"],
                                "lapack_residual": lapack["residual"], "lapack_orth": lapack["orth"]}


def main():
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(16, os.cpu_count() or 1)
    with multiprocessing.Pool(jobs) as pool:
        out = dict(pool.map(record, sorted(GPU_CALLS, key=lambda c: -c[1]), chunksize=1))
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    with open(R.GOLDEN, "w") as f:
        json.dump({k: out[k] for k in sorted(out)}, f, indent=1)
        f.write("\n")
    worst = {k: max(v[k] for v in out.values()) for k in ("sweeps", "residual", "orth", "eig", "lapack_residual", "lapack_orth")}
    print(len(out), "cases; worst:", worst)


if __name__ == "__main__":
    main()
