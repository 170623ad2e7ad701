#!/usr/bin/env python3
"""Measurements behind profiles/ttft_quantile.md (run from the repository root
on a machine with an MI355X and the built extensions).

  python tools/ttft_quantile_bench.py roundtrip OUT.json
      submit + collect wall clock of the quantile kernel, of the waiting-time
      tail kernel on the same rows, and of the native host quantile solver.
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- \\
      python tools/ttft_quantile_bench.py launches
      the same launches and nothing else, for a kernel trace of its own;
  python tools/ttft_quantile_bench.py summarize DIR/.../*_kernel_trace.csv OUT.json
      kernel-only times per (kernel, B, N) from that trace.
  python tools/ttft_quantile_bench.py parity OUT.json
      worst oracle error over the bound of every implementation on the
      known-answer table of tests/test_ops_ttft_quantile.py.

Shapes: B = 192, 4096 x N = 256, 700, the rows of tools/ttft_tail_bench.py
(TTFT targets uniform in 300...3000 ms, which only the tail kernel reads),
eps = 0.05 and per-replica rates uniform in 0.98...1 of the rate range's
maximum: there more than 5 % of the arrivals wait on every row, so the search
over t runs on every row (``searched`` in the round trip's output counts them;
at half the maximum rate it runs on about one row in ten, and the others end
after the mean evaluation).
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
KERNELS = ("wva_quantile_kernel", "wva_solve_kernel_tail")
WARMUP, REPS = 3, 30


def rows(b, n):
    rng = np.random.default_rng(7)
    p = np.zeros((b, 12))
    p[:, :7] = (4.137, 0.027, 5.2, 0.0011, 512, 128, n)
    p[:, 7] = rng.uniform(300.0, 3000.0, b)  # TTFT targets, ms
    p[:, 10] = rng.uniform(10.0, 500.0, b)
    p[:, 11] = 1
    service = 5.2 + 0.0011 * 512 * n + 127 * (4.137 + 0.027 * n)
    rate_max = n / service * (1 - 0.001) * 1000.0  # req/s
    rates = np.random.default_rng(13).uniform(0.98, 1.0, b) * rate_max
    return p, rates, np.full(b, 0.05)


def timed(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(ts), "median_ms": float(np.median(ts)), "max_ms": max(ts)}


def launchers(native, p, n, rates, eps):
    return {"quantile_kernel": lambda: native.collect(native.submit_quantile(p, n, rates, eps)),
            "tail_kernel": lambda: native.collect(native.submit_tail(p, n, eps))}


def roundtrip(out_path):
    from wva_amd import ops

    native, cpu = ops.get_native(), ops.get_native_cpu()
    out = []
    for b, n in SHAPES:
        p, rates, eps = rows(b, n)
        res = native.collect(native.submit_quantile(p, n, rates, eps))
        ref = cpu.ttft_quantiles(p, rates, eps)
        # a row whose search did not run has q = prefill, what eps close to 1 gives
        prefill = cpu.ttft_quantiles(p, rates, np.full(b, 1 - 1e-12))[:, 1]
        rec = {"B": b, "N": n, "valid": int(res[:, 0].sum()),
               "valid_mismatch_vs_host": int((res[:, 0] != ref[:, 0]).sum()),
               "searched": int((ref[:, 1] > prefill).sum()),
               "q_max_rel_vs_host": float(np.abs(res[:, 1] / ref[:, 1] - 1).max())}
        for name, fn in launchers(native, p, n, rates, eps).items():
            rec[name] = timed(fn)
        rec["host_quantile"] = timed(lambda: cpu.ttft_quantiles(p, rates, eps), reps=5)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def launches():
    from wva_amd import ops

    native = ops.get_native()
    for b, n in SHAPES:
        p, rates, eps = rows(b, n)
        for fn in launchers(native, p, n, rates, eps).values():
            for _ in range(WARMUP + REPS):
                fn()


def summarize(trace_path, out_path):
    """Kernel-only times from the trace of ``launches``: its dispatches, in
    start order, are WARMUP + REPS of each of the two kernels for each shape
    (the trace does not tell N: the tables are in dynamic LDS).  The last REPS
    of each run, end - start."""
    runs = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                   int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                  for r in csv.DictReader(open(trace_path))
                  if r["Kernel_Name"].split(".")[0] in KERNELS)
    per = WARMUP + REPS
    plan = [(b, n, k) for b, n in SHAPES for k in KERNELS]
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


def parity(out_path):
    import test_ops_ttft_quantile as T
    import torch

    cases = [c for c in T.table() if c["tol"] is not None]
    args = T.arrays(cases)
    want = np.array([c["t"] for c in cases])
    tol = np.array([c["tol"] for c in cases])
    prefill = np.array([c["prefill"] for c in cases])
    out = {}
    for k, solve in T.IMPLS.items():
        if k.startswith("kernel") and not torch.cuda.is_available():
            continue
        t_got = (solve(*args)[:, 1] - prefill) / ((1 + args[3]) / 2)
        err = np.abs(t_got / want - 1)
        out[k] = {"worst_t_rel_err": float(err.max()),
                  "worst_err_over_bound": float((err / tol).max()),
                  "at_N": int(args[0][int(np.argmax(err / tol)), 6]), "cases": len(cases)}
    print(json.dumps(out, indent=1))
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    {"roundtrip": roundtrip, "launches": launches, "summarize": summarize,
     "parity": parity}[sys.argv[1]](*sys.argv[2:])
