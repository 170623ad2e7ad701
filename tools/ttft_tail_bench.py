#!/usr/bin/env python3
"""Measurements behind profiles/ttft_tail.md and profiles/ttft_tail_large_n.md
(run from the repository root on a machine with an MI355X and the built
extensions).  SET is one of the shape sets below and defaults to ``small``,
the set of profiles/ttft_tail.md.

  python tools/ttft_tail_bench.py roundtrip OUT.json [SET]
      submit + collect wall clock of the set's kernels and of the native host
      solvers on the same rows.
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- \\
      python tools/ttft_tail_bench.py launches [SET]
      the same launches and nothing else, for a kernel trace of its own;
  python tools/ttft_tail_bench.py summarize DIR/.../*_kernel_trace.csv OUT.json [SET]
      kernel-only times per (kernel, B, N) from that trace.
  python tools/ttft_tail_bench.py parity OUT.json [SET]
      worst rate_star error of every implementation on the known-answer
      table of tests/test_ops_ttft_tail.py (``large``:
      tests/test_ops_ttft_tail_large_n.py), and the same with the vector
      dropped.
  python tools/ttft_tail_bench.py cycle [STEPS]
      one JSON line: the sizing cycle of the oversized-N1024 fleet
      (tests/fleet_oracle.py) under WVA_TTFT_PERCENTILE=95, 2 chunks,
      large_n on.

Shape sets:
  small  B = 192, 4096 x N = 256, 700: the tail kernel against the 256-thread
         mean kernel (TTFT targets uniform in 300...3000 ms);
  cross  the same shapes and rows: the compact tail kernel against the tail
         kernel;
  large  B = 192, 4096 x N = 1024, 7680: the compact tail kernel against the
         compact mean kernel, TTFT targets between 0.05 and 3 times
         (1024 / N)^1.5 full-batch service times above the full-batch prefill,
         so that the search binds on every row.
"""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))

SMALL_SHAPES = [(b, n) for b in (192, 4096) for n in (256, 700)]
LARGE_SHAPES = [(b, n) for b in (192, 4096) for n in (1024, 7680)]
WARMUP, REPS = 3, 30


def rows(b, n):
    rng = np.random.default_rng(7)
    p = np.zeros((b, 12))
    p[:, :7] = (4.137, 0.027, 5.2, 0.0011, 512, 128, n)
    p[:, 7] = rng.uniform(300.0, 3000.0, b)  # TTFT targets, ms
    p[:, 10] = rng.uniform(10.0, 500.0, b)
    p[:, 11] = 1
    return p, np.full(b, 0.05)


def rows_binding(b, n):
    p, eps = rows(b, n)
    prefill = 5.2 + 0.0011 * 512 * n
    service = prefill + 127 * (4.137 + 0.027 * n)
    # near lam_max about 1000 requests wait, whatever N is: a wait of about
    # 1000 / N service times, so the window of targets that bind shrinks
    # with N.  The exponent was picked on the host reference: with 1.5 every
    # row of every shape binds (with 1.0, 132 of 192 at N = 7680).
    spread = service * (1024.0 / n) ** 1.5
    p[:, 7] = prefill + np.random.default_rng(11).uniform(0.05, 3.0, b) * spread
    return p, eps


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


def cross_launchers(native, p, n, eps):
    return {"tail_compact_kernel": lambda: native.collect(native.submit_tail_compact(p, n, eps)),
            "tail_kernel": lambda: native.collect(native.submit_tail(p, n, eps))}


def large_launchers(native, p, n, eps):
    return {"tail_compact_kernel": lambda: native.collect(native.submit_tail_compact(p, n, eps)),
            "compact_mean_kernel": lambda: native.collect(native.submit_compact(p, n))}


# name -> (shapes, rows, launchers, the launchers' kernels in the trace, the
# entry point whose results are compared with the host solver's)
SETS = {
    "small": (SMALL_SHAPES, rows, launchers,
              ("wva_solve_kernel_tail", "wva_solve_kernel_256"), "submit_tail"),
    "cross": (SMALL_SHAPES, rows, cross_launchers,
              ("wva_solve_kernel_tail_compact", "wva_solve_kernel_tail"), "submit_tail_compact"),
    "large": (LARGE_SHAPES, rows_binding, large_launchers,
              ("wva_solve_kernel_tail_compact", "wva_solve_kernel_compact"),
              "submit_tail_compact"),
}


def roundtrip(out_path, which="small"):
    from wva_amd import ops

    shapes, make_rows, make_launchers, _, entry = SETS[which]
    native, cpu = ops.get_native(), ops.get_native_cpu()
    out = []
    for b, n in shapes:
        p, eps = make_rows(b, n)
        res = native.collect(getattr(native, entry)(p, n, eps))
        ref = cpu.solve_allocations(p, None, eps)
        feas = res[:, 0] == 1
        rec = {"B": b, "N": n, "feasible": int(feas.sum()),
               "replica_mismatch_vs_host": int((res[:, 1] != ref[:, 1]).sum()),
               "rate_star_max_rel_vs_host": float(np.abs(res[feas, 2] / ref[feas, 2] - 1).max())}
        if which != "small":
            # the search binds where lam* stays below lam_max (its rate_star is
            # the largest of the launch: the rows differ in the target alone)
            rec["search_binds"] = int((res[feas, 2] < res[feas, 2].max() * (1 - 1e-9)).sum())
            own = cpu.solve_allocations_tail_compact(p, None, eps)
            rec["replica_mismatch_vs_host_reference"] = int((res[:, 1] != own[:, 1]).sum())
            rec["rate_star_max_rel_vs_host_reference"] = float(
                np.abs(res[feas, 2] / own[feas, 2] - 1).max())
            rec["host_tail_compact"] = timed(
                lambda: cpu.solve_allocations_tail_compact(p, None, eps), reps=5)
        for name, fn in make_launchers(native, p, n, eps).items():
            rec[name] = timed(fn)
        rec["host_tail"] = timed(lambda: cpu.solve_allocations(p, None, eps), reps=5)
        rec["host_mean"] = timed(lambda: cpu.solve_allocations(p), reps=5)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def launches(which="small"):
    from wva_amd import ops

    shapes, make_rows, make_launchers, _, _ = SETS[which]
    native = ops.get_native()
    for b, n in shapes:
        p, eps = make_rows(b, n)
        for fn in make_launchers(native, p, n, eps).values():
            for _ in range(WARMUP + REPS):
                fn()


def summarize(trace_path, out_path, which="small"):
    """Kernel-only times from the trace of ``launches``: its dispatches, in
    start order, are WARMUP + REPS of each of the set's two kernels for each
    shape (the trace does not tell N: the tables are in dynamic LDS).  The
    last REPS of each run, end - start."""
    shapes, _, _, kernels, _ = SETS[which]
    runs = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                   int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                  for r in csv.DictReader(open(trace_path)) if "wva_solve_kernel" in r["Kernel_Name"])
    per = WARMUP + REPS
    plan = [(b, n, k) for b, n in shapes for k in kernels]
    assert len(runs) == per * len(plan), (len(runs), per * len(plan))
    out = []
    for i, (b, n, kernel) in enumerate(plan):
        chunk = runs[i * per:(i + 1) * per]
        assert all(name.split(".")[0] == kernel and wg == b for _, _, name, wg in chunk), (b, n, kernel)
        us = np.array([end - start for start, end, _, _ in chunk[-REPS:]]) / 1e3
        out.append({"kernel": kernel, "B": b, "N": n, "min_us": float(us.min()),
                    "median_us": float(np.median(us)), "max_us": float(us.max())})
        print(json.dumps(out[-1]))
    json.dump(out, open(out_path, "w"), indent=1)


def parity(out_path, which="small"):
    import torch

    if which == "large":
        import test_ops_ttft_tail_large_n as T

        impls = {k: (solve, cases()) for k, (solve, cases) in T.IMPLS.items()}
        drop = lambda p, scv: T.CPU.solve_allocations(p, scv)  # noqa: E731
    else:
        import test_ops_ttft_tail as T

        impls = {k: (solve, T.table()) for k, solve in T.IMPLS.items()}
        drop = T.IMPLS["cpu"]
    out = {}
    for k, (solve, table) in impls.items():
        if k.startswith("kernel") and not torch.cuda.is_available():
            continue
        cases = [c for c in table if c["rate_tol"] not in (None, T.FINAL_TOL)]
        p, scv, eps = T.arrays(cases)
        want = np.array([float(c["rate_star"]) for c in cases])
        tol = np.array([c["rate_tol"] for c in cases])
        err = np.abs(solve(p, scv, eps)[:, 2] / want - 1)
        out[k] = {"worst_rate_star_rel_err": float(err.max()),
                  "worst_err_over_bound": float((err / tol).max()),
                  "at_N": int(p[int(np.argmax(err / tol)), 6]), "cases": len(cases)}
    cases = [c for c in next(iter(impls.values()))[1] if c["rate_tol"] not in (None, T.FINAL_TOL)]
    p, scv, _ = T.arrays(cases)
    want = np.array([float(c["rate_star"]) for c in cases])
    tol = np.array([c["rate_tol"] for c in cases])
    dropped = np.abs(drop(p, scv)[:, 2] / want - 1)
    out["vector_dropped(cpu)"] = {"cases_outside_bound": int((dropped > tol).sum()),
                                  "cases": len(cases),
                                  "smallest_err_over_bound": float((dropped / tol).min())}
    print(json.dumps(out, indent=1))
    json.dump(out, open(out_path, "w"), indent=1)


def cycle(steps="300"):
    import fleet_oracle as fo
    from test_cycle_oracle import new_system, sizing_env
    from wva_amd.ops import BatchedAllocationSolver

    fleet = fo.oversized_fleet()
    with sizing_env(fleet, "gpu") as mp:
        mp.setenv("WVA_TTFT_PERCENTILE", "95")
        system = new_system(fleet)
        solver = BatchedAllocationSolver(device="cuda", chunks=2, large_n=True)
        ts = []
        for i in range(30 + int(steps)):
            t0 = time.perf_counter()
            solver.calculate(system)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts[30:])
    print(json.dumps({"fleet": fleet.name, "rows": fleet.rows(), "chunks": 2, "steps": len(ts),
                      "median_ms": float(np.median(ts)), "min_ms": float(ts.min()),
                      "p95_ms": float(np.percentile(ts, 95))}))


if __name__ == "__main__":
    {"roundtrip": roundtrip, "launches": launches, "summarize": summarize,
     "parity": parity, "cycle": cycle}[sys.argv[1]](*sys.argv[2:])
