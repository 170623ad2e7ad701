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

Every command but ``host`` takes a last argument ``large`` for the shapes of
profiles/ttft_quantile_large_n.md: the compact quantile kernel against the
compact tail kernel at B = 192, 4096 x N = 701, 1024, 7680, and both quantile
kernels at N = 256, 700; ``large`` may be followed by the lower end of the
rates' range as a fraction of the maximum (default 0.98).

  python tools/ttft_quantile_bench.py host OUT.json [LOW]
      the native host quantile solver alone on the large shapes: also runs on
      an older build (from its directory, with this file's path).

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
LARGE_SHAPES = [(b, n) for b in (192, 4096) for n in (256, 700, 701, 1024, 7680)]
WARMUP, REPS = 3, 30


def large_kernels(n):
    """The two kernels of a large shape, in launch order."""
    if n <= 700:
        return ("wva_quantile_kernel", "wva_quantile_kernel_compact")
    return ("wva_quantile_kernel_compact", "wva_solve_kernel_tail_compact")


def rows(b, n, low=0.98):
    rng = np.random.default_rng(7)
    p = np.zeros((b, 12))
    p[:, :7] = (4.137, 0.027, 5.2, 0.0011, 512, 128, n)
    p[:, 7] = rng.uniform(300.0, 3000.0, b)  # TTFT targets, ms
    p[:, 10] = rng.uniform(10.0, 500.0, b)
    p[:, 11] = 1
    service = 5.2 + 0.0011 * 512 * n + 127 * (4.137 + 0.027 * n)
    rate_max = n / service * (1 - 0.001) * 1000.0  # req/s
    rates = np.random.default_rng(13).uniform(float(low), 1.0, b) * rate_max
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


def large_launchers(native, p, n, rates, eps):
    compact = lambda: native.collect(native.submit_quantile_compact(p, n, rates, eps))
    if n <= 700:
        return {"quantile_kernel": lambda: native.collect(native.submit_quantile(p, n, rates, eps)),
                "quantile_kernel_compact": compact}
    return {"quantile_kernel_compact": compact,
            "tail_kernel_compact": lambda: native.collect(native.submit_tail_compact(p, n, eps))}


def searched(cpu, p, rates, ref):
    # a row whose search did not run has q = prefill, what eps close to 1 gives
    prefill = cpu.ttft_quantiles(p, rates, np.full(len(p), 1 - 1e-12))[:, 1]
    return int((ref[:, 1] > prefill).sum())


def roundtrip_large(out_path, low):
    from wva_amd import ops

    native, cpu = ops.get_native(), ops.get_native_cpu()
    out = []
    for b, n in LARGE_SHAPES:
        p, rates, eps = rows(b, n, low)
        res = native.collect(native.submit_quantile_compact(p, n, rates, eps))
        ref = cpu.ttft_quantiles(p, rates, eps)
        ref_compact = cpu.ttft_quantiles_compact(p, rates, eps)
        rel = lambda a, b_: float(np.abs(a[:, 1] / b_[:, 1] - 1).max())
        rec = {"B": b, "N": n, "low": float(low), "valid": int(res[:, 0].sum()),
               "valid_mismatch_vs_host": int((res[:, 0] != ref[:, 0]).sum()),
               "searched": searched(cpu, p, rates, ref),
               "q_max_rel_kernel_vs_host_compact": rel(res, ref_compact),
               "q_max_rel_kernel_vs_host": rel(res, ref),
               "q_max_rel_host_compact_vs_host": rel(ref_compact, ref)}
        for name, fn in large_launchers(native, p, n, rates, eps).items():
            rec[name] = timed(fn, reps=REPS if b * n < 4096 * 7680 else 10)
        rec["host_quantile"] = timed(lambda: cpu.ttft_quantiles(p, rates, eps), reps=5)
        rec["host_quantile_compact"] = timed(lambda: cpu.ttft_quantiles_compact(p, rates, eps),
                                             reps=5)
        out.append(rec)
        print(json.dumps(rec), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def host(out_path, low=0.98):
    from wva_amd import ops

    cpu = ops.get_native_cpu()
    out = []
    for b, n in LARGE_SHAPES:
        p, rates, eps = rows(b, n, low)
        out.append({"B": b, "N": n, "low": float(low),
                    "host_quantile": timed(lambda: cpu.ttft_quantiles(p, rates, eps), reps=5)})
        print(json.dumps(out[-1]), flush=True)
    json.dump(out, open(out_path, "w"), indent=1)


def roundtrip(out_path, which="small", low=0.98):
    from wva_amd import ops

    if which == "large":
        return roundtrip_large(out_path, low)
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


def launches(which="small", low=0.98):
    from wva_amd import ops

    native = ops.get_native()
    for b, n in (LARGE_SHAPES if which == "large" else SHAPES):
        p, rates, eps = rows(b, n, low)
        pick = large_launchers if which == "large" else launchers
        for fn in pick(native, p, n, rates, eps).values():
            for _ in range(WARMUP + REPS):
                fn()


def summarize(trace_path, out_path, which="small"):
    """Kernel-only times from the trace of ``launches``: its dispatches, in
    start order, are WARMUP + REPS of each of the two kernels for each shape
    (the trace does not tell N: the tables are in dynamic LDS).  The last REPS
    of each run, end - start."""
    runs = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                   int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                  for r in csv.DictReader(open(trace_path))
                  if r["Kernel_Name"].split(".")[0] in KERNELS + large_kernels(701))
    per = WARMUP + REPS
    plan = [(b, n, k) for b, n in SHAPES for k in KERNELS]
    if which == "large":
        plan = [(b, n, k) for b, n in LARGE_SHAPES for k in large_kernels(n)]
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
    import test_ops_ttft_quantile as T
    import torch

    table, impls = T.table, T.IMPLS
    if which == "large":
        import test_ops_ttft_quantile_large_n as L

        table, impls = L.table, L.IMPLS
    cases = [c for c in table() if c["tol"] is not None]
    args = T.arrays(cases)
    want = np.array([c["t"] for c in cases])
    tol = np.array([c["tol"] for c in cases])
    prefill = np.array([c["prefill"] for c in cases])
    out = {}
    for k, solve in impls.items():
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
     "parity": parity, "host": host}[sys.argv[1]](*sys.argv[2:])
