"""Timing of the ITL-percentile sizing kernel (``submit_ptile``).

Rows whose ITL search binds (``target_itl`` half a step above decode_time(N -
1), ``itl_tail = 0.05``) at B in (192, 4096) and N in (256, 700, 1024, 7680):

- ``ptile``: the round trip through ``submit_ptile``;
- ``split``: the same through ``submit_ptile(split=True)``, the rejected
  arrangement with the TTFT and ITL searches side by side on one wave each;
- ``mean``: the same rows sized to the mean on ``submit`` (N <= 700) or
  ``submit_compact``: what the percentile costs;
- ``host``: the same percentile rows through ``solve_allocations_ptile`` of the
  torch-free binding.

Prints one JSON line per cell with the median and range of ``--steps`` round
trips in ms.  Kernel-only times come from running this script under
``rocprofv3 --kernel-trace``; every cell launches its kernel warmup + steps
times, in the order printed.
"""

import argparse
import json
import statistics
import time

import numpy as np

from wva_amd import ops


def rows(batch, n):
    beta = 0.027 if n <= 1000 else 0.0002
    row = np.zeros(12)
    row[:7] = (4.137, beta, 5.2, 0.0011, 512, 128, n)
    row[8] = 4.137 + beta * (n - 1) + beta / 2
    row[10], row[11] = 50.0, 1.0
    p = np.tile(row, (batch, 1))
    p[:, 10] *= 1.0 + np.arange(batch) / batch  # distinct loads, same search
    return p


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    samples = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        samples.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the host route")
    args = ap.parse_args()
    native, cpu = ops.get_native(), ops.get_native_cpu()
    for batch in (192, 4096):
        for n in (256, 700, 1024, 7680):
            p = rows(batch, n)
            itl = np.full(batch, 0.05)
            mean = (lambda: native.collect(native.submit(p, 11 * n))) if n <= 700 else (
                lambda: native.collect(native.submit_compact(p, n)))
            cells = {"ptile": lambda: native.collect(native.submit_ptile(p, n, itl)),
                     "split": lambda: native.collect(native.submit_ptile(p, n, itl, None, None, True)),
                     "mean": mean}
            if args.host:
                cells["host"] = lambda: cpu.solve_allocations_ptile(p, None, None, itl)
            for name, fn in cells.items():
                print(json.dumps({"cell": name, "B": batch, "N": n,
                                  **timed(fn, args.warmup, args.steps)}), flush=True)


if __name__ == "__main__":
    main()
