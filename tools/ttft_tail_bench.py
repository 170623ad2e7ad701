#!/usr/bin/env python3
"""Measurements behind profiles/ttft_tail.md (run from the repository root on
a machine with an MI355X and the built extensions).

  python tools/ttft_tail_bench.py roundtrip OUT.json
      submit + collect wall clock of the tail kernel, the 256-thread mean
      kernel and the native host solver on the same rows.
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- \\
      python tools/ttft_tail_bench.py launches
      the same launches and nothing else, for a kernel trace of its own;
  python tools/ttft_tail_bench.py summarize DIR/.../*_kernel_trace.csv OUT.json
      kernel-only times per (kernel, B, N) from that trace.
  python tools/ttft_tail_bench.py parity OUT.json
      worst rate_star error of every implementation on the known-answer
      table of tests/test_ops_ttft_tail.py, and the same with the vector
      dropped.
"""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))

SHAPES = [(b, n) for b in (192, 4096) for n in (256, 700)]
WARMUP, REPS = 3, 30


def rows(b, n):
    rng = np.random.default_rng(7)
    p = np.zeros((b, 12))
    p[:, :7] = (4.137, 0.027, 5.2, 0.0011, 512, 128, n)
    p[:, 7] = rng.uniform(300.0, 3000.0, b)  # TTFT targets, ms
    p[:, 10] = rng.uniform(10.0, 500.0, b)
    p[:, 11] = 1
    return p, np.full(b, 0.05)


def timed(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": float(np.median(ts)), "max_ms": max(ts)}


def launchers(native, p, n, eps):
    def mean_256():
        os.environ["WVA_GPU_THREADS"] = "256"  # read per launch
        try:
            return native.collect(native.submit(p, 11 * n))
        finally:
            del os.environ["WVA_GPU_THREADS"]

    return {"tail_kernel": lambda: native.collect(native.submit_tail(p, n, eps)),
            "mean_kernel_256": mean_256}


def roundtrip(out_path):
    from wva_amd import ops

    native, cpu = ops.get_native(), ops.get_native_cpu()
    out = []
    for b, n in SHAPES:
        p, eps = rows(b, n)
        res, ref = native.collect(native.submit_tail(p, n, eps)), cpu.solve_allocations(p, None, eps)
        feas = res[:, 0] == 1
        rec = {"B": b, "N": n, "feasible": int(feas.sum()),
               "replica_mismatch_vs_host": int((res[:, 1] != ref[:, 1]).sum()),
               "rate_star_max_rel_vs_host": float(np.abs(res[feas, 2] / ref[feas, 2] - 1).max())}
        for name, fn in launchers(native, p, n, eps).items():
            rec[name] = timed(fn)
        rec["host_tail"] = timed(lambda: cpu.solve_allocations(p, None, eps), reps=5)
        rec["host_mean"] = timed(lambda: cpu.solve_allocations(p), reps=5)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def launches():
    from wva_amd import ops

    native = ops.get_native()
    for b, n in SHAPES:
        p, eps = rows(b, n)
        for fn in launchers(native, p, n, eps).values():
            for _ in range(WARMUP + REPS):
                fn()


def summarize(trace_path, out_path):
    """Kernel-only times from the trace of ``launches``: its dispatches, in
    start order, are WARMUP + REPS of the tail kernel and then of the mean
    kernel for each shape in SHAPES (the trace does not tell N: the tables
    are in dynamic LDS).  The last REPS of each run, end - start."""
    runs = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                   int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                  for r in csv.DictReader(open(trace_path)) if "wva_solve_kernel" in r["Kernel_Name"])
    per = WARMUP + REPS
    plan = [(b, n, k) for b, n in SHAPES for k in ("wva_solve_kernel_tail", "wva_solve_kernel_256")]
    assert len(runs) == per * len(plan), (len(runs), per * len(plan))
    out = []
    for i, (b, n, kernel) in enumerate(plan):
        chunk = runs[i * per:(i + 1) * per]
        assert all(name.startswith(kernel) and wg == b for _, _, name, wg in chunk), (b, n, kernel)
        us = np.array([end - start for start, end, _, _ in chunk[-REPS:]]) / 1e3
        out.append({"kernel": kernel, "B": b, "N": n, "min_us": float(us.min()),
                    "median_us": float(np.median(us)), "max_us": float(us.max())})
        print(json.dumps(out[-1]))
    json.dump(out, open(out_path, "w"), indent=1)


def parity(out_path):
    import torch

    import test_ops_ttft_tail as T

    cases = [c for c in T.table() if c["rate_tol"] not in (None, T.FINAL_TOL)]
    p, scv, eps = T.arrays(cases)
    want = np.array([float(c["rate_star"]) for c in cases])
    tol = np.array([c["rate_tol"] for c in cases])
    out = {}
    for k in T.IMPLS:
        if k.startswith("kernel") and not torch.cuda.is_available():
            continue
        err = np.abs(T.IMPLS[k](p, scv, eps)[:, 2] / want - 1)
        out[k] = {"worst_rate_star_rel_err": float(err.max()),
                  "worst_err_over_bound": float((err / tol).max()),
                  "at_N": int(p[int(np.argmax(err / tol)), 6]), "cases": len(cases)}
    dropped = np.abs(T.IMPLS["cpu"](p, scv)[:, 2] / want - 1)
    out["vector_dropped(cpu)"] = {"cases_outside_bound": int((dropped > tol).sum()),
                                  "cases": len(cases),
                                  "smallest_err_over_bound": float((dropped / tol).min())}
    print(json.dumps(out, indent=1))
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    {"roundtrip": roundtrip, "launches": launches, "summarize": summarize,
     "parity": parity}[sys.argv[1]](*sys.argv[2:])
