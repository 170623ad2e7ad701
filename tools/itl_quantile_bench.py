#!/usr/bin/env python3
"""Measurements behind profiles/itl_quantile.md (run from the repository root
on a machine with an MI355X and the built extensions).

  python tools/itl_quantile_bench.py roundtrip OUT.json
      submit + collect wall clock of the ITL quantile kernel, of the TTFT
      quantile kernel on the same rows (submit_quantile up to N = 700,
      submit_quantile_compact above), and of the native host itl_quantiles.
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- \\
      python tools/itl_quantile_bench.py launches
      the same launches and nothing else, for a kernel trace of its own;
  python tools/itl_quantile_bench.py summarize DIR/.../*_kernel_trace.csv OUT.json
      kernel-only times per (kernel, B, N) from that trace.

Shapes: B = 192, 4096 x N = 256, 700, 7680, the rows, rates (0.98...1 of the
rate range's maximum) and eps = 0.05 of tools/ttft_quantile_bench.py.  The ITL
kernel's work does not depend on the rate; the TTFT kernels search on every
such row.
"""
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ttft_quantile_bench import REPS, WARMUP, rows, timed  # noqa: E402

SHAPES = [(b, n) for b in (192, 4096) for n in (256, 700, 7680)]


def ttft_kernel(n):
    return "wva_quantile_kernel" if n <= 700 else "wva_quantile_kernel_compact"


def launchers(native, p, n, rates, eps):
    ttft = native.submit_quantile if n <= 700 else native.submit_quantile_compact
    return {"wva_itl_quantile_kernel":
            lambda: native.collect(native.submit_itl_quantile(p, n, rates, eps)),
            ttft_kernel(n): lambda: native.collect(ttft(p, n, rates, eps))}


def roundtrip(out_path):
    from wva_amd import ops

    native, cpu = ops.get_native(), ops.get_native_cpu()
    out = []
    for b, n in SHAPES:
        p, rates, eps = rows(b, n)
        res = native.collect(native.submit_itl_quantile(p, n, rates, eps))
        ref = cpu.itl_quantiles(p, rates, eps)
        rec = {"B": b, "N": n, "valid": int(res[:, 0].sum()),
               "rows_differing_from_host": int((res != ref).any(axis=1).sum())}
        for name, fn in launchers(native, p, n, rates, eps).items():
            rec[name] = timed(fn, reps=REPS if b * n < 4096 * 7680 else 10)
        rec["host_itl_quantiles"] = timed(lambda: cpu.itl_quantiles(p, rates, eps), reps=5)
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
    start order, are WARMUP + REPS of each of the two kernels for each shape.
    The last REPS of each run, end - start."""
    names = {"wva_itl_quantile_kernel", "wva_quantile_kernel", "wva_quantile_kernel_compact"}
    runs = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                   int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
                  for r in csv.DictReader(open(trace_path))
                  if r["Kernel_Name"].split(".")[0] in names)
    per = WARMUP + REPS
    plan = [(b, n, k) for b, n in SHAPES for k in ("wva_itl_quantile_kernel", ttft_kernel(n))]
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


if __name__ == "__main__":
    {"roundtrip": roundtrip, "launches": launches,
     "summarize": summarize}[sys.argv[1]](*sys.argv[2:])
