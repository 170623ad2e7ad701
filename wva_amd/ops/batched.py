"""Batched allocation sizing over a whole System.

The reference sizes one (server, accelerator) pair at a time inside the
reconcile loop (hot loop #1: /root/reference/pkg/core/server.go:55-67 ->
allocation.go:27-163).  Here the analyze phase is *batched*: all pairs of
the fleet are packed into one [B, 12] float64 matrix and solved either by
the native extension (the torch-free C++/OpenMP binding on CPU, or the
gfx950 HIP kernel — one workgroup per pair) or by the pure-Python
analyzer fallback.  M/G/1-corrected sizing (a per-row service-time cs^2,
below) runs on the same native paths: ``BatchedAllocationSolver`` resolves
each server's cs^2 and hands the vector to ``solve_problems(..., scv=...)``.
Only a bare ``solve_problems(problems)`` under ``WVA_ANALYZER=mg1`` — no
explicit ``scv`` — still routes through the scalar Python analyzer with the
environment's fleet value.  On the GPU the matrix travels through the native
submit/collect dispatch (csrc/sizing_dispatch.h), and
``BatchedAllocationSolver`` may cut the fleet into chunks so that its own
per-row host work overlaps the launches (docs/design/native-queue-solver.md).
Rows whose max batch exceeds GPU_MAX_BATCH_LIMIT leave the GPU for the CPU
solver unless the ``large_n`` opt-in (``WVA_GPU_LARGE_N=1``) sends them to the
compact-table kernel (same document, "Compact table").

Field layouts mirror wva_amd/csrc/queue_core.h, and so does the row
contract (``row_valid`` there, ``valid_rows`` here).  A row is valid iff

- every field is finite;
- alpha, beta, gamma, delta >= 0;
- trunc(N) >= 1 and the chain length 11 * N fits a C int;
- trunc(out_tokens) >= 1 (and fits a C int);
- in_tokens >= 0;
- every target >= 0.

An invalid row yields the all-zero result row in every implementation, as
the analyzer's ``check()`` methods reject it.  in_tokens, out_tokens, N and
min_replicas are truncated toward zero, so replica counts are integral.

M/G/1 correction (per-row service-time cs^2; ``valid_scv`` here):

- a sizing row may carry a service-time cs^2, ``scv``;
- ``wait_scale = (1 + scv) / 2``;
- TTFT is ``wait * wait_scale + prefill(eff_conc)`` wherever it is
  evaluated: in the bisection and in the final ``R_TTFT``;
- nothing else changes; the ``wait >= 0`` clamp stays before the scaling;
- ``scv`` must be finite and ``>= 0``; any other value gives the all-zero
  result row in every implementation (``QueueAnalyzer`` rejects ``scv < 0``,
  the native guard also rejects NaN and inf);
- the ``-1`` sentinel means "use the fleet value"; it is resolved on the
  host, and a kernel never sees it;
- the 12-column problem layout and the 6-column result layout do not
  change: ``scv`` travels as a separate optional float64 vector of length B.

No vector, or a vector of all 1.0, gives results bit-identical to the
Markovian ones on every path.

TTFT percentile (per-row waiting-time tail; ``valid_tail`` here):

- a sizing row may carry ``ttft_tail = eps``, the allowed probability that
  TTFT exceeds ``target_ttft`` (p95 is ``eps = 0.05``);
- ``eps = 0`` means "mean TTFT": the search compares the mean TTFT with the
  target, as it always did;
- for ``eps > 0`` the TTFT search runs on ``y(lam) = P(W > t(lam))`` against
  the target value ``eps``, with ``t(lam) = (target_ttft -
  prefill(eff_conc(lam))) / wait_scale`` and ``y = 1`` when ``t <= 0``;
  ``QueueAnalyzer.wait_exceedance`` is the definition of ``P(W > t)``;
- the ITL search, the TPS back-off, the replica count and the final
  evaluation do not change, and ``R_TTFT`` stays the predicted *mean* TTFT
  at the final rate: only lam* moves, and through it the replica count;
- ``eps`` must be finite with ``0 <= eps < 1``; any other value gives the
  all-zero result row in every implementation;
- a row with ``target_ttft = 0`` ignores a valid ``eps``;
- the layouts do not change: ``eps`` travels as a separate optional float64
  vector of length B, like ``scv``.

No vector, or a vector of all 0, gives results bit-identical to the ones
without it on every path.  On the GPU the rows with ``eps > 0`` and a TTFT
target run on the waiting-time tail kernel (``submit_tail``, N up to
GPU_MAX_BATCH_LIMIT), a second launch next to the one every other row takes
unchanged.  Such rows with a larger N go to the native CPU solver, unless the
``large_n`` opt-in is on: then those up to GPU_COMPACT_MAX_BATCH_LIMIT run on
the compact waiting-time tail kernel (``submit_tail_compact``: the same model
and window, the tail sum by the Poisson recurrence instead of a log-factorial
table), one more launch enqueued before any is collected.  Routes of a GPU
solve with a ``ttft_tail`` vector:

- eps > 0, target_ttft > 0, N <= 700: ``submit_tail``;
- the same with 700 < N <= 7680, ``large_n`` on, not under ``WVA_GPU_GRAPH=1``:
  ``submit_tail_compact``;
- the same with ``large_n`` off (the default), or N > 7680: native CPU solver;
- every other row: the route it takes without the vector.

The TTFT each allocation exceeds at that percentile is predicted afterwards,
by ``ttft_quantiles`` (one call per cycle).  Its routes on the GPU:

- N <= 700: ``submit_quantile``;
- 700 < N <= 7680, ``large_n`` on, not under ``WVA_GPU_GRAPH=1``:
  ``submit_quantile_compact`` (the quantile search without a table of the tail
  sum), one more launch, enqueued before anything is collected;
- the same with ``large_n`` off (the default), or N > 7680: native CPU solver
  while the launches run.

ITL percentile (per-row occupancy tail; ``valid_tail`` here as well):

- a sizing row may carry ``itl_tail = eps``, the allowed fraction of tokens
  whose ITL exceeds ``target_itl`` (p95 is ``eps = 0.05``);
- ``eps = 0`` means "mean ITL": the search compares the decode time at the
  mean effective concurrency with the target, as it always did;
- for ``eps > 0`` the ITL search runs on the token-weighted share of decode
  steps slower than ``target_itl`` against the target value ``eps``;
  ``QueueAnalyzer.itl_exceedance`` is its definition;
- the TTFT search (mean or ``ttft_tail``), the TPS back-off, the replica count
  and the final evaluation do not change, and ``R_ITL`` stays the predicted
  *mean* ITL at the final rate;
- ``eps`` must be finite with ``0 <= eps < 1``; any other value gives the
  all-zero result row in every implementation;
- a row with ``target_itl = 0`` ignores a valid ``eps``;
- the layouts do not change: ``eps`` travels as a separate optional float64
  vector of length B, and composes with ``scv`` and ``ttft_tail`` on a row.

No vector, or a vector of all 0, gives results bit-identical to the ones
without it on every path, through the code that ran before.  Routes of a GPU
solve with an ``itl_tail`` vector (``_PtileTicket``):

- eps > 0, target_itl > 0, N <= 700: ``submit_ptile``, one more ticket enqueued
  before any is collected; the row's ``ttft_tail`` rides along;
- the same with 700 < N <= 7680, ``large_n`` on, not under ``WVA_GPU_GRAPH=1``:
  a second ``submit_ptile`` launch;
- the same with ``large_n`` off, N > 7680, or under ``WVA_GPU_GRAPH=1``:
  ``solve_allocations_ptile`` on the CPU while the launches run;
- every other row: the route it takes without the vector; an invalid eps
  gives the all-zero row.

ITL quantile.  The ITL each allocation's tokens exceed at that share is
predicted afterwards, by ``itl_quantiles`` (one call per cycle), for the rows
with an ITL target: with ``S_b`` the share of tokens emitted in decode steps
with more than b requests in service, ``b* = min{b in 1..N : S_b <= eps}`` and
the quantile is ``decode_time(b*)``; ``QueueAnalyzer.itl_quantile`` is the
definition.  The rate is fixed, so the native paths find b* in one sweep over
the states and a scan, without a search.  There is no ``scv``.  Its routes on
the GPU:

- N <= 700: ``submit_itl_quantile``, one launch; invalid rows ride along;
- 700 < N <= 7680, ``large_n`` on, not under ``WVA_GPU_GRAPH=1``: a second
  ``submit_itl_quantile`` launch that reserves LDS for those rows alone,
  enqueued before anything is collected;
- the same with ``large_n`` off (the default), or N > 7680: native CPU solver
  while the launches run.
"""

from __future__ import annotations

import contextlib
import copy
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from ..analyzer import (
    AnalyzerError,
    Configuration,
    DecodeParms,
    PrefillParms,
    QueueAnalyzer,
    RequestSize,
    ServiceParms,
    TargetPerf,
    configured_itl_tail,
    configured_ttft_tail,
    percentile_ttft_tail,
)
from ..config import MAX_QUEUE_TO_BATCH_RATIO
from ..core import Allocation, System
from ..core.allocation import _zero_load_allocation, energy_value_term

# problem columns
P_ALPHA, P_BETA, P_GAMMA, P_DELTA = 0, 1, 2, 3
P_IN_TOKENS, P_OUT_TOKENS, P_MAX_BATCH = 4, 5, 6
P_TARGET_TTFT, P_TARGET_ITL, P_TARGET_TPS = 7, 8, 9
P_TOTAL_RATE, P_MIN_REPLICAS = 10, 11
PROBLEM_FIELDS = 12

# result columns
R_FEASIBLE, R_REPLICAS, R_RATE_STAR, R_ITL, R_TTFT, R_RHO = range(6)
RESULT_FIELDS = 6

# columns of a ttft_quantiles row: 1.0 for a row that got a value, and the
# TTFT quantile in ms (0 is a legitimate one)
Q_VALID, Q_TTFT = range(2)
QUANTILE_FIELDS = 2
# an itl_quantiles row has the same shape: the ITL quantile in ms in column 1
Q_ITL = Q_TTFT

# the GPU path keeps the cumulative table in LDS: N <= ~700
GPU_MAX_BATCH_LIMIT = 700

# the compact-table kernel keeps only cum[0..N-1] there (csrc/queue_core.h):
# N + 256 + 64 doubles in 64 KiB allow 7872, rounded down to a multiple of 256
GPU_COMPACT_MAX_BATCH_LIMIT = 7680

# largest N whose chain length 11 * N fits a C int (queue_core.h kMaxBatchLimit)
_MAX_BATCH_LIMIT = (2**31 - 1) // (1 + MAX_QUEUE_TO_BATCH_RATIO)


def valid_rows(problems: np.ndarray) -> np.ndarray:
    """Boolean mask of the rows that satisfy the row contract (module
    docstring); the same predicate as ``row_valid`` in csrc/queue_core.h."""
    p = problems
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(axis=1)
        ok &= (p[:, P_ALPHA : P_DELTA + 1] >= 0).all(axis=1)
        ok &= (p[:, P_MAX_BATCH] >= 1) & (p[:, P_MAX_BATCH] < _MAX_BATCH_LIMIT + 1)
        ok &= (p[:, P_OUT_TOKENS] >= 1) & (p[:, P_OUT_TOKENS] < 2.0**31)
        ok &= p[:, P_IN_TOKENS] >= 0
        ok &= (p[:, P_TARGET_TTFT : P_TARGET_TPS + 1] >= 0).all(axis=1)
    return ok


def valid_scv(scv: np.ndarray) -> np.ndarray:
    """Boolean mask of the service-time cs^2 values a row may carry: finite
    and >= 0 (the ``scv`` part of ``row_valid`` in csrc/queue_core.h).  The
    ``-1`` sentinel fails it: it must be resolved before a solver sees it."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(scv) & (scv >= 0)


def valid_tail(ttft_tail: np.ndarray) -> np.ndarray:
    """Boolean mask of the TTFT tail probabilities a row may carry: finite
    with 0 <= eps < 1 (the ``tail_eps`` part of ``row_valid`` in
    csrc/queue_core.h)."""
    with np.errstate(invalid="ignore"):
        return (ttft_tail >= 0) & (ttft_tail < 1)


def _scv_vector(scv, n_rows: int, name: str = "scv") -> np.ndarray:
    """An explicit ``scv`` (or ``ttft_tail``) — a scalar for the whole batch
    or a float64 ``[B]`` array — as the C-contiguous float64 ``[B]`` vector
    the native bindings take.  An array of another dtype or shape raises, as
    the bindings do."""
    if isinstance(scv, np.ndarray) and scv.ndim > 0:
        if scv.dtype != np.float64:
            raise TypeError(f"{name} must be float64, got {scv.dtype}")
        if scv.shape != (n_rows,):
            raise ValueError(f"{name} must be a scalar or [B] = [{n_rows}], got {scv.shape}")
        return np.ascontiguousarray(scv)
    return np.full(n_rows, float(scv), dtype=np.float64)


# hipGraph dispatch cache: repeated fleet solves of the same shape replay
# a captured graph instead of re-launching.  Keyed by (B, max_k, whether the
# launch carries a cs^2 vector); replays copy fresh problem data (and the
# fresh cs^2 vector) into the captured input buffers.  Opt-in via
# WVA_GPU_GRAPH=1: the fleet solve is ONE kernel, so launch overhead is
# ~1% of the dispatch and replay measured no win (0.96 vs 0.94 ms
# headline cycle) — the path exists for launch-bound configurations
# (many small heterogeneous dispatches), not the default.  Any capture
# failure falls back to plain dispatch permanently (logged once).
_graph_cache: dict = {}
_graph_lock = None
_graph_disabled = False
_mg1_warned = False


def _graph_requested() -> bool:
    return not _graph_disabled and os.environ.get("WVA_GPU_GRAPH", "0") == "1"


def _large_n_requested(large_n: Optional[bool]) -> bool:
    """Whether rows with GPU_MAX_BATCH_LIMIT < N <= GPU_COMPACT_MAX_BATCH_LIMIT
    go to the compact-table kernel instead of the CPU split: the caller's
    ``large_n``, or for ``None`` the environment (``WVA_GPU_LARGE_N=1``, read
    per call).  Off by default.  The hipGraph route keeps the CPU split."""
    if large_n is None:
        large_n = os.environ.get("WVA_GPU_LARGE_N", "0") == "1"
    return bool(large_n) and not _graph_requested()


_NO_DEVICE_SWITCH = contextlib.nullcontext()


def _on_device(device):
    """Context that makes ``device`` current for the native dispatch (which
    runs on the current device); plain "cuda" already is."""
    if str(device) == "cuda":
        return _NO_DEVICE_SWITCH
    import torch

    return torch.cuda.device(torch.device(device))


def _graph_solve(native, problems_t, max_k, scv_t=None):
    """Solve via a cached hipGraph; None -> caller uses plain dispatch.
    ``scv_t`` is the optional device vector of per-row cs^2."""
    global _graph_lock, _graph_disabled
    import threading

    if _graph_disabled or os.environ.get("WVA_GPU_GRAPH", "0") != "1":
        return None
    import torch

    if _graph_lock is None:
        _graph_lock = threading.Lock()
    key = (problems_t.shape[0], max_k, scv_t is not None)
    with _graph_lock:
        entry = _graph_cache.get(key)
        try:
            if entry is None:
                if len(_graph_cache) >= 16:
                    # bound the private graph memory pools when fleet
                    # shapes churn; oldest capture goes first
                    _graph_cache.pop(next(iter(_graph_cache)))
                static_in = problems_t.clone()
                static_scv = scv_t.clone() if scv_t is not None else None
                # warm up on a side stream (capture requires a clean stream)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    native.solve_allocations(static_in, max_k, static_scv)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = native.solve_allocations(static_in, max_k, static_scv)
                _graph_cache[key] = (graph, static_in, static_scv, static_out)
                # capture only RECORDS the work — replay to actually run
                # it for this call's data
                graph.replay()
                return static_out.cpu().numpy()
            graph, static_in, static_scv, static_out = entry
            static_in.copy_(problems_t)
            if static_scv is not None:
                static_scv.copy_(scv_t)
            graph.replay()
            return static_out.cpu().numpy()
        except Exception as e:  # pragma: no cover - depends on ROCm graph support
            _graph_disabled = True
            import logging

            logging.getLogger("wva").warning(
                "hipGraph dispatch unavailable; using plain launches: %s", e
            )
            return None


class _LargeNTicket:
    """One chunk split by max batch N (the ``large_n`` opt-in), in flight.

    - rows with N <= GPU_MAX_BATCH_LIMIT, and invalid rows, went to
      ``native.submit`` with the max_k of those rows alone, so they get the
      geometry and the results they get without the opt-in, bit for bit;
    - valid rows up to GPU_COMPACT_MAX_BATCH_LIMIT went to
      ``native.submit_compact`` as a second launch;
    - valid rows beyond that were solved on the CPU while both launches ran.

    Each part carried the cs^2 of its own rows.  ``collect`` waits for both
    launches and merges the three parts back in row order."""

    def __init__(self, native, device, problems, batch_limits, scv_arr):
        n_rows = problems.shape[0]
        small = batch_limits <= GPU_MAX_BATCH_LIMIT
        big = batch_limits > GPU_COMPACT_MAX_BATCH_LIMIT
        middle = ~(small | big)
        self.n_rows = n_rows
        self.parts = []  # (row mask, native ticket)
        self.big = big
        self.big_solved = None

        def part(mask):
            rows = np.ascontiguousarray(problems[mask])
            return rows, (None if scv_arr is None else np.ascontiguousarray(scv_arr[mask]))

        try:
            with _on_device(device):
                if small.any():
                    rows, scv = part(small)
                    # solve_problems' max_k rule on these rows alone: the raw
                    # column unless an invalid row's N is a NaN or too large
                    max_batch = rows[:, P_MAX_BATCH].max()
                    if not max_batch <= GPU_MAX_BATCH_LIMIT:
                        max_batch = batch_limits[small].max()
                    max_k = max(int(max_batch), 1) * (1 + MAX_QUEUE_TO_BATCH_RATIO)
                    args = (rows, max_k) if scv is None else (rows, max_k, scv)
                    self.parts.append((small, native.submit(*args)))
                if middle.any():
                    rows, scv = part(middle)
                    max_n = int(batch_limits[middle].max())
                    args = (rows, max_n) if scv is None else (rows, max_n, scv)
                    self.parts.append((middle, native.submit_compact(*args)))
            if big.any():
                rows, scv = part(big)
                if scv is None:
                    self.big_solved = solve_problems(rows, device="cpu")
                else:
                    self.big_solved = solve_problems(rows, device="cpu", scv=scv)
        except BaseException:
            # a launch already enqueued must not keep its slot for good
            for _, ticket in self.parts:
                try:
                    native.collect(ticket)
                except Exception:
                    pass
            raise

    def collect(self, native) -> np.ndarray:
        out = np.empty((self.n_rows, RESULT_FIELDS), dtype=np.float64)
        parts, self.parts = self.parts, []
        error = None
        for mask, ticket in parts:  # every ticket is collected, whatever happens
            try:
                out[mask] = native.collect(ticket)
            except Exception as e:  # pragma: no cover - needs a failing GPU
                error = error or e
        if error is not None:
            raise error
        if self.big_solved is not None:
            out[self.big] = self.big_solved
        return out


class _TailTicket:
    """One chunk split by TTFT functional (a ``ttft_tail`` vector), in flight.

    - valid rows with ``eps > 0``, a TTFT target and N <= GPU_MAX_BATCH_LIMIT
      went to ``native.submit_tail``, enqueued first;
    - with ``large_n`` (the opt-in, already resolved by the caller), such rows
      with GPU_MAX_BATCH_LIMIT < N <= GPU_COMPACT_MAX_BATCH_LIMIT went to
      ``native.submit_tail_compact``, one more launch enqueued right behind;
    - every other row went to ``submit_rest`` without a vector: today's
      route, with today's max_k and geometry pick, bit for bit (a row whose
      eps is invalid rides along and is zeroed in the merge);
    - the remaining tail rows (N above the limit of the launches allowed; all
      tail rows under ``WVA_GPU_GRAPH=1``) were solved by the native CPU
      solver while the launches ran.

    Each part carried the cs^2 of its own rows.  ``collect`` waits for every
    part and merges them back in row order."""

    def __init__(self, native, device, problems, tail_arr, scv_arr, submit_rest, collect_rest,
                 large_n=False):
        self.native = native
        self.n_rows = problems.shape[0]
        self.collect_rest = collect_rest
        self.bad = ~valid_tail(tail_arr)
        with np.errstate(invalid="ignore"):
            wants = valid_rows(problems) & ~self.bad & (tail_arr > 0)
            wants &= problems[:, P_TARGET_TTFT] > 0
            on_kernel = wants & (problems[:, P_MAX_BATCH] <= GPU_MAX_BATCH_LIMIT)
            on_compact = wants & ~on_kernel & (problems[:, P_MAX_BATCH] <= GPU_COMPACT_MAX_BATCH_LIMIT)
        if _graph_requested():
            on_kernel = np.zeros_like(wants)
        if not large_n or _graph_requested():
            on_compact = np.zeros_like(wants)
        self.on_kernel, self.on_compact, self.rest = on_kernel, on_compact, ~wants
        self.on_cpu = wants & ~on_kernel & ~on_compact
        self.kernel_ticket = self.compact_ticket = self.rest_ticket = self.cpu_solved = None

        def part(mask):
            rows = np.ascontiguousarray(problems[mask])
            return rows, (None if scv_arr is None else np.ascontiguousarray(scv_arr[mask]))

        def submit_tail_rows(submit, mask):
            rows, scv = part(mask)
            max_n = int(rows[:, P_MAX_BATCH].max())
            args = (rows, max_n, np.ascontiguousarray(tail_arr[mask]))
            with _on_device(device):
                return submit(*(args if scv is None else args + (scv,)))

        try:
            if on_kernel.any():
                self.kernel_ticket = submit_tail_rows(native.submit_tail, on_kernel)
            if on_compact.any():
                self.compact_ticket = submit_tail_rows(native.submit_tail_compact, on_compact)
            if self.rest.any():
                self.rest_ticket = submit_rest(*part(self.rest))
            if self.on_cpu.any():
                rows, scv = part(self.on_cpu)
                extra = {} if scv is None else {"scv": scv}
                self.cpu_solved = solve_problems(
                    rows, device="cpu", ttft_tail=np.ascontiguousarray(tail_arr[self.on_cpu]), **extra
                )
        except BaseException:
            # a launch already enqueued must not keep its slot for good
            try:
                self.collect()
            except Exception:
                pass
            raise

    def collect(self) -> np.ndarray:
        out = np.zeros((self.n_rows, RESULT_FIELDS), dtype=np.float64)
        kernel_ticket, self.kernel_ticket = self.kernel_ticket, None
        compact_ticket, self.compact_ticket = self.compact_ticket, None
        rest_ticket, self.rest_ticket = self.rest_ticket, None
        error = None
        try:  # every ticket is collected, whatever happens
            if rest_ticket is not None:
                out[self.rest] = self.collect_rest(rest_ticket)
        except Exception as e:  # pragma: no cover - needs a failing GPU
            error = e
        for mask, ticket in ((self.on_kernel, kernel_ticket), (self.on_compact, compact_ticket)):
            try:
                if ticket is not None:
                    out[mask] = self.native.collect(ticket)
            except Exception as e:  # pragma: no cover - needs a failing GPU
                error = error or e
        if error is not None:
            raise error
        if self.cpu_solved is not None:
            out[self.on_cpu] = self.cpu_solved
        out[self.bad] = 0.0
        return out


def _ptile_rows(problems: np.ndarray, itl_arr: np.ndarray) -> np.ndarray:
    """Mask of the rows whose ITL search runs on the occupancy tail: valid,
    with a valid ``itl_tail`` > 0 and an ITL target."""
    with np.errstate(invalid="ignore"):
        return (valid_rows(problems) & valid_tail(itl_arr) & (itl_arr > 0)
                & (problems[:, P_TARGET_ITL] > 0))


def _masked(mask, problems, *vectors):
    """The rows of ``mask`` and the same rows of each optional vector,
    C-contiguous; a vector that is None stays None."""
    return (np.ascontiguousarray(problems[mask]),
            *(None if v is None else np.ascontiguousarray(v[mask]) for v in vectors))


class _PtileTicket:
    """One chunk split by ITL functional (an ``itl_tail`` vector), in flight.

    - ``_ptile_rows`` with N <= GPU_MAX_BATCH_LIMIT went to
      ``native.submit_ptile``, enqueued first, with their ``ttft_tail`` and cs^2;
    - with ``large_n`` (already resolved by the caller), such rows with
      GPU_MAX_BATCH_LIMIT < N <= GPU_COMPACT_MAX_BATCH_LIMIT went to a second
      ``native.submit_ptile`` launch, which reserves LDS for their N alone;
    - every other row went to ``submit_rest(rows, scv, ttft_tail)``: the route
      it takes without the vector, bit for bit (a row whose ``itl_tail`` is
      invalid rides along and is zeroed in the merge);
    - the remaining percentile rows (N above the limit of the launches allowed;
      all of them under ``WVA_GPU_GRAPH=1``) were solved by the native CPU
      solver while the launches ran.

    ``collect`` waits for every part and merges them back in row order."""

    def __init__(self, native, device, problems, itl_arr, tail_arr, scv_arr, submit_rest,
                 collect_rest, large_n=False):
        self.native = native
        self.n_rows = problems.shape[0]
        self.collect_rest = collect_rest
        self.bad = ~valid_tail(itl_arr)
        wants = _ptile_rows(problems, itl_arr)
        small = wants & (problems[:, P_MAX_BATCH] <= GPU_MAX_BATCH_LIMIT)
        middle = wants & ~small & (problems[:, P_MAX_BATCH] <= GPU_COMPACT_MAX_BATCH_LIMIT)
        if _graph_requested():
            small = np.zeros_like(wants)
        if not large_n or _graph_requested():
            middle = np.zeros_like(wants)
        self.rest, self.on_cpu = ~wants, wants & ~small & ~middle
        self.tickets = []  # (row mask, native ticket)
        self.rest_ticket = self.cpu_solved = None

        def part(mask):
            return _masked(mask, problems, scv_arr, tail_arr)

        try:
            for mask in (small, middle):
                if mask.any():
                    rows, scv, tail = part(mask)
                    with _on_device(device):
                        self.tickets.append((mask, native.submit_ptile(
                            rows, int(rows[:, P_MAX_BATCH].max()),
                            np.ascontiguousarray(itl_arr[mask]), tail, scv)))
            if self.rest.any():
                self.rest_ticket = submit_rest(*part(self.rest))
            if self.on_cpu.any():
                rows, scv, tail = part(self.on_cpu)
                extra = {} if scv is None else {"scv": scv}
                self.cpu_solved = solve_problems(
                    rows, device="cpu", ttft_tail=tail,
                    itl_tail=np.ascontiguousarray(itl_arr[self.on_cpu]), **extra)
        except BaseException:
            # a launch already enqueued must not keep its slot for good
            try:
                self.collect()
            except Exception:
                pass
            raise

    def collect(self) -> np.ndarray:
        out = np.zeros((self.n_rows, RESULT_FIELDS), dtype=np.float64)
        tickets, self.tickets = self.tickets, []
        rest_ticket, self.rest_ticket = self.rest_ticket, None
        error = None
        try:  # every ticket is collected, whatever happens
            if rest_ticket is not None:
                out[self.rest] = self.collect_rest(rest_ticket)
        except Exception as e:  # pragma: no cover - needs a failing GPU
            error = e
        for mask, ticket in tickets:
            try:
                out[mask] = self.native.collect(ticket)
            except Exception as e:  # pragma: no cover - needs a failing GPU
                error = error or e
        if error is not None:
            raise error
        if self.cpu_solved is not None:
            out[self.on_cpu] = self.cpu_solved
        out[self.bad] = 0.0
        return out


def _solve_ptile_host(problems, device, scv_arr, tail_arr, itl_arr) -> np.ndarray:
    """``solve_problems`` off the GPU with an ``itl_tail`` vector: the
    ``_ptile_rows`` through ``solve_allocations_ptile`` of the torch-free
    binding, else of the torch binding, else through the Python analyzer; every
    other row by the call it gets without the vector."""
    from . import get_native, get_native_cpu, native_available, native_cpu_available

    out = np.zeros((problems.shape[0], RESULT_FIELDS), dtype=np.float64)
    wants = _ptile_rows(problems, itl_arr)

    def part(mask):
        return _masked(mask, problems, scv_arr, tail_arr)

    if wants.any():
        rows, scv, tail = part(wants)
        itl = np.ascontiguousarray(itl_arr[wants])
        if native_cpu_available():
            out[wants] = get_native_cpu().solve_allocations_ptile(rows, scv, tail, itl)
        elif native_available():
            import torch

            out[wants] = get_native().solve_allocations_ptile(
                torch.from_numpy(rows), *(None if v is None else torch.from_numpy(v)
                                          for v in (scv, tail, itl))).numpy()
        else:
            from . import warn_if_pure_python_fallback

            warn_if_pure_python_fallback()
            out[wants] = _solve_problems_python(
                rows, 1.0 if scv is None else scv, 0.0 if tail is None else tail, itl)
    if not wants.all():
        rows, scv, tail = part(~wants)
        extra = {} if scv is None else {"scv": scv}
        out[~wants] = solve_problems(rows, device, ttft_tail=tail, **extra)
    out[~valid_tail(itl_arr)] = 0.0
    return out


def _valid_batch_limits(problems: np.ndarray) -> np.ndarray:
    """Column N with the invalid rows' entries replaced by 1, so that they
    neither size a launch nor leave the GPU."""
    return np.where(valid_rows(problems), problems[:, P_MAX_BATCH], 1.0)


def _solve_problems_python(problems: np.ndarray, scv=1.0, ttft_tail=0.0,
                           itl_tail=0.0) -> np.ndarray:
    """Reference-semantics scalar fallback via the Python analyzer.

    ``scv`` is the service-time cs^2 — a scalar for the whole batch or a
    per-row float64 array (mg1 auto mode derives one per server); a row
    whose cs^2 fails ``valid_scv`` yields the all-zero row.  ``ttft_tail``
    is the TTFT tail probability, a scalar or per-row likewise; a row whose
    value fails ``valid_tail`` yields the all-zero row.  ``itl_tail`` is the
    ITL tail fraction under the same rules."""
    scv_arr = _scv_vector(scv, problems.shape[0])
    tail_arr = _scv_vector(ttft_tail, problems.shape[0], "ttft_tail")
    itl_arr = _scv_vector(itl_tail, problems.shape[0], "itl_tail")
    out = np.zeros((problems.shape[0], RESULT_FIELDS), dtype=np.float64)
    valid = valid_rows(problems) & valid_scv(scv_arr) & valid_tail(tail_arr) & valid_tail(itl_arr)
    for i, row in enumerate(problems):
        if not valid[i]:
            continue  # all-zero row; also keeps int() off NaN and inf
        N = int(row[P_MAX_BATCH])
        config = Configuration(
            max_batch_size=N,
            max_queue_size=N * MAX_QUEUE_TO_BATCH_RATIO,
            service_parms=ServiceParms(
                prefill=PrefillParms(gamma=row[P_GAMMA], delta=row[P_DELTA]),
                decode=DecodeParms(alpha=row[P_ALPHA], beta=row[P_BETA]),
            ),
        )
        try:
            qa = QueueAnalyzer(
                config,
                RequestSize(
                    avg_input_tokens=int(row[P_IN_TOKENS]),
                    avg_output_tokens=int(row[P_OUT_TOKENS]),
                ),
                scv=float(scv_arr[i]),
            )
            _, metrics, _ = qa.size(
                TargetPerf(
                    target_ttft=row[P_TARGET_TTFT],
                    target_itl=row[P_TARGET_ITL],
                    target_tps=row[P_TARGET_TPS],
                    ttft_tail=float(tail_arr[i]),
                    itl_tail=float(itl_arr[i]),
                )
            )
            rate_star = metrics.throughput
            total_rate = row[P_TOTAL_RATE]
            n_rep = max(math.ceil(total_rate / rate_star), int(row[P_MIN_REPLICAS]))
            if n_rep <= 0:
                continue  # no replicas: no per-replica rate to analyze
            final = qa.analyze(total_rate / n_rep)  # rejects rate <= 0
        except AnalyzerError:
            continue
        out[i, R_FEASIBLE] = 1.0
        out[i, R_REPLICAS] = n_rep
        out[i, R_RATE_STAR] = rate_star
        out[i, R_ITL] = final.avg_token_time
        out[i, R_TTFT] = final.avg_wait_time + final.avg_prefill_time
        out[i, R_RHO] = final.rho
    return out


def solve_problems(
    problems: np.ndarray, device: Optional[str] = None, scv=None,
    large_n: Optional[bool] = None, ttft_tail=None, itl_tail=None,
) -> np.ndarray:
    """Solve a [B, 12] problem matrix -> [B, 6] results.

    device: None for automatic (native CPU if built, else Python), "cpu" to
    force the native/Python CPU path, or a torch device string like "cuda"
    to run the gfx950 kernel.

    scv: None, or the service-time cs^2 of the M/G/1 correction (module
    docstring) — a scalar for the whole batch or a float64 ``[B]`` array.
    An explicit ``scv`` never reads the environment and runs on the native
    paths (GPU dispatch, else the torch-free binding, else the torch
    binding; the Python analyzer only when nothing native is built).
    ``None`` is the Markovian model, except under ``WVA_ANALYZER=mg1``,
    where the environment's fleet value goes through the Python analyzer.

    large_n: on the GPU, whether valid rows with GPU_MAX_BATCH_LIMIT < N <=
    GPU_COMPACT_MAX_BATCH_LIMIT run on the compact-table kernel (a second
    launch, enqueued together with the first) instead of the CPU.  ``None``
    asks the environment (``WVA_GPU_LARGE_N=1``), ``False`` forces the CPU
    split.  Off by default; no effect on the CPU, on rows within
    GPU_MAX_BATCH_LIMIT, or under ``WVA_GPU_GRAPH=1``.  It covers percentile
    rows (``ttft_tail``) as well: those run on the compact tail kernel.

    ttft_tail: None, or the TTFT tail probability of the percentile sizing
    (module docstring) — a scalar for the whole batch or a float64 ``[B]``
    array.  None and all zeros are the mean TTFT, on today's routes.
    Otherwise, on the GPU, the rows with ``eps > 0``, a TTFT target and N <=
    GPU_MAX_BATCH_LIMIT run on the waiting-time tail kernel, a second launch
    enqueued before the first is collected; tail rows with a larger N go to
    the compact tail kernel up to GPU_COMPACT_MAX_BATCH_LIMIT when ``large_n``
    is on and to the native CPU solver otherwise (all tail rows under
    ``WVA_GPU_GRAPH=1``), and every other row takes the route it takes
    without the vector.

    itl_tail: None, or the ITL tail fraction of the percentile sizing (module
    docstring, "ITL percentile") — a scalar for the whole batch or a float64
    ``[B]`` array.  None and all zeros are the mean ITL, on today's routes and
    through today's code.  Otherwise the rows with ``eps > 0`` and an ITL
    target run on the percentile kernel (``submit_ptile``) or, where the
    module docstring's table says so, on ``solve_allocations_ptile`` on the
    CPU; every other row takes the route it takes without the vector.
    """
    from . import get_native, native_available

    problems = np.ascontiguousarray(problems, dtype=np.float64)
    if problems.ndim != 2 or problems.shape[1] != PROBLEM_FIELDS:
        raise ValueError(f"problems must be [B, {PROBLEM_FIELDS}]")
    scv_arr = None if scv is None else _scv_vector(scv, problems.shape[0])
    tail_arr = None
    if ttft_tail is not None:
        tail_arr = _scv_vector(ttft_tail, problems.shape[0], "ttft_tail")
        if not tail_arr.any():
            tail_arr = None  # all zeros: the mean TTFT, today's routes
    itl_arr = None
    if itl_tail is not None:
        itl_arr = _scv_vector(itl_tail, problems.shape[0], "itl_tail")
        if not itl_arr.any():
            itl_arr = None  # all zeros: the mean ITL, today's routes
    if problems.shape[0] == 0:
        return np.zeros((0, RESULT_FIELDS), dtype=np.float64)

    from ..analyzer.mg1 import configured_scv

    env_scv = 1.0 if scv_arr is not None else configured_scv()
    if env_scv != 1.0:
        scv = env_scv
        # WVA_ANALYZER=mg1: the Allen-Cunneen wait scaling lives in the
        # Python analyzer; the native kernels implement the Markovian
        # contract only, so mg1 mode routes through the scalar path
        # (opt-in capacity-planning mode, not the hot default); callers
        # that want the native paths pass the cs^2 explicitly
        global _mg1_warned
        if not _mg1_warned:
            _mg1_warned = True
            import logging

            logging.getLogger("wva_amd.ops").info(
                "WVA_ANALYZER=mg1 (cs^2=%.3g): sizing via the Python "
                "M/G/1-corrected analyzer instead of the native kernel", scv,
            )
        return _solve_problems_python(
            problems, scv=scv, ttft_tail=0.0 if tail_arr is None else tail_arr,
            itl_tail=0.0 if itl_arr is None else itl_arr,
        )

    want_gpu = device is not None and str(device).startswith("cuda")
    if itl_arr is not None and not want_gpu:
        return _solve_ptile_host(problems, device, scv_arr, tail_arr, itl_arr)
    if want_gpu and (tail_arr is not None or itl_arr is not None):
        native = get_native()  # raises loudly if missing on a GPU box

        def submit_rest(rows, rows_scv):
            """Today's route for the other rows.  Where that is the lean
            dispatch (no row above GPU_MAX_BATCH_LIMIT, no hipGraph), only its
            submit half, with the same max_k: both launches are enqueued
            before either is collected.  Any other route runs on the spot."""
            extra = () if rows_scv is None else (rows_scv,)
            max_batch = rows[:, P_MAX_BATCH].max()
            if max_batch <= GPU_MAX_BATCH_LIMIT and not _graph_requested():
                max_k = max(int(max_batch), 1) * (1 + MAX_QUEUE_TO_BATCH_RATIO)
                with _on_device(device):
                    return native.submit(rows, max_k, *extra), None
            named = {} if rows_scv is None else {"scv": rows_scv}
            return None, solve_problems(rows, device, large_n=large_n, **named)

        def collect_rest(ticket):
            return ticket[1] if ticket[0] is None else native.collect(ticket[0])

        if itl_arr is None:
            split = _TailTicket(native, device, problems, tail_arr, scv_arr, submit_rest,
                                collect_rest, large_n=_large_n_requested(large_n))
            return split.collect()

        def submit_other(rows, rows_scv, rows_tail):
            """The rows the percentile kernel does not take: a ``_TailTicket``
            where some carry a ``ttft_tail``, ``submit_rest`` otherwise."""
            if rows_tail is None or not rows_tail.any():
                return submit_rest(rows, rows_scv)
            return _TailTicket(native, device, rows, rows_tail, rows_scv, submit_rest,
                               collect_rest, large_n=_large_n_requested(large_n))

        def collect_other(ticket):
            return ticket.collect() if isinstance(ticket, _TailTicket) else collect_rest(ticket)

        split = _PtileTicket(native, device, problems, itl_arr, tail_arr, scv_arr, submit_other,
                             collect_other, large_n=_large_n_requested(large_n))
        return split.collect()
    if want_gpu:
        native = get_native()  # raises loudly if missing on a GPU box
        import torch

        # the kernel's row guard turns invalid rows into zero rows, so they
        # ride along; only when the largest N is a NaN or past the LDS
        # limit is the predicate needed here, to keep invalid rows from
        # sizing the launch or being sent to the CPU path
        batch_limits = problems[:, P_MAX_BATCH]
        max_batch = batch_limits.max()
        if not max_batch <= GPU_MAX_BATCH_LIMIT:
            batch_limits = np.where(valid_rows(problems), batch_limits, 1.0)
            max_batch = batch_limits.max()
        if max_batch > GPU_MAX_BATCH_LIMIT and _large_n_requested(large_n):
            # opt-in: a second, compact-table launch takes the rows up to
            # GPU_COMPACT_MAX_BATCH_LIMIT; only rows beyond it leave the GPU
            split = _LargeNTicket(native, device, problems, batch_limits, scv_arr)
            return split.collect(native)
        if max_batch > GPU_MAX_BATCH_LIMIT:
            # LDS-resident limit: solve oversized problems on CPU
            big = batch_limits > GPU_MAX_BATCH_LIMIT
            out = np.empty((problems.shape[0], RESULT_FIELDS), dtype=np.float64)
            if scv_arr is None:
                out[~big] = solve_problems(problems[~big], device=device)
                out[big] = solve_problems(problems[big], device="cpu")
            else:  # each part takes the cs^2 of its own rows
                out[~big] = solve_problems(problems[~big], device=device, scv=scv_arr[~big])
                out[big] = solve_problems(problems[big], device="cpu", scv=scv_arr[big])
            return out
        # chain length computed host-side (also feeds hipGraph capture,
        # where the binding's device-sync fallback is illegal)
        max_k = max(int(max_batch), 1) * (1 + MAX_QUEUE_TO_BATCH_RATIO)
        if _graph_requested():
            t = torch.from_numpy(problems).to(device)
            scv_t = None if scv_arr is None else torch.from_numpy(scv_arr).to(device)
            res = _graph_solve(native, t, max_k, scv_t)
            if res is not None:
                return res
        # lean dispatch (csrc/sizing_dispatch.h): pinned staging, no output
        # fill, no tensors — here as one chunk, submitted and collected
        with _on_device(device):
            if scv_arr is None:
                return native.collect(native.submit(problems, max_k))
            return native.collect(native.submit(problems, max_k, scv_arr))

    from . import get_native_cpu, native_cpu_available

    if native_cpu_available():
        # torch-free binding: same host solver as the torch binding
        # (bit-identical; csrc/queue_host.h) but measured ~6x faster on
        # CPU — plain OpenMP beats at::parallel_for's per-call overhead
        # on this workload (profiles/r01_torchfree_cpu.json) — and it is
        # the only native path in the slim controller image.
        if tail_arr is not None:
            return get_native_cpu().solve_allocations(problems, scv_arr, tail_arr)
        if scv_arr is None:
            return get_native_cpu().solve_allocations(problems)
        return get_native_cpu().solve_allocations(problems, scv_arr)
    if native_available():
        import torch

        native = get_native()
        if tail_arr is not None:
            return native.solve_allocations(
                torch.from_numpy(problems), -1,
                None if scv_arr is None else torch.from_numpy(scv_arr),
                torch.from_numpy(tail_arr),
            ).numpy()
        if scv_arr is None:
            return native.solve_allocations(torch.from_numpy(problems)).numpy()
        return native.solve_allocations(
            torch.from_numpy(problems), -1, torch.from_numpy(scv_arr)
        ).numpy()
    from . import warn_if_pure_python_fallback

    warn_if_pure_python_fallback()
    if tail_arr is not None:
        return _solve_problems_python(
            problems, scv=1.0 if scv_arr is None else scv_arr, ttft_tail=tail_arr
        )
    if scv_arr is None:
        return _solve_problems_python(problems)
    return _solve_problems_python(problems, scv=scv_arr)


def _row_analyzer(row, scv: float = 1.0) -> QueueAnalyzer:
    """The ``QueueAnalyzer`` of a row that passed ``valid_rows``."""
    N = int(row[P_MAX_BATCH])
    config = Configuration(
        max_batch_size=N,
        max_queue_size=N * MAX_QUEUE_TO_BATCH_RATIO,
        service_parms=ServiceParms(
            prefill=PrefillParms(gamma=row[P_GAMMA], delta=row[P_DELTA]),
            decode=DecodeParms(alpha=row[P_ALPHA], beta=row[P_BETA]),
        ),
    )
    size = RequestSize(avg_input_tokens=int(row[P_IN_TOKENS]),
                       avg_output_tokens=int(row[P_OUT_TOKENS]))
    return QueueAnalyzer(config, size, scv=scv)


def _ttft_quantiles_python(problems, rates, eps, scv) -> np.ndarray:
    """``ttft_quantiles`` row by row through ``QueueAnalyzer.ttft_quantile``,
    the semantic reference; a rejected row is ``(0, 0)``."""
    out = np.zeros((problems.shape[0], QUANTILE_FIELDS), dtype=np.float64)
    valid = valid_rows(problems) & valid_scv(scv)
    for i, row in enumerate(problems):
        if not valid[i]:
            continue
        try:
            qa = _row_analyzer(row, float(scv[i]))
            out[i] = 1.0, qa.ttft_quantile(float(rates[i]), float(eps[i]))
        except AnalyzerError:
            continue
    return out


def _itl_quantiles_python(problems, rates, eps) -> np.ndarray:
    """``itl_quantiles`` row by row through ``QueueAnalyzer.itl_quantile``,
    the semantic reference; a rejected row is ``(0, 0)``."""
    out = np.zeros((problems.shape[0], QUANTILE_FIELDS), dtype=np.float64)
    valid = valid_rows(problems)
    for i, row in enumerate(problems):
        if not valid[i]:
            continue
        try:
            out[i] = 1.0, _row_analyzer(row).itl_quantile(float(rates[i]), float(eps[i]))
        except AnalyzerError:
            continue
    return out


def ttft_quantiles(problems: np.ndarray, rates, eps, device: Optional[str] = None,
                   scv=None, large_n: Optional[bool] = None) -> np.ndarray:
    """The TTFT each row exceeds with probability ``eps`` at the per-replica
    rate ``rates`` (req/s): [B, 12] problems -> [B, 2] of ``(Q_VALID, Q_TTFT)``
    (csrc/queue_core.h, "TTFT quantile"; ``QueueAnalyzer.ttft_quantile`` is
    the definition).  ``eps = 0.05`` asks for the p95 TTFT in ms.

    ``rates``, ``eps`` and the optional ``scv`` follow ``_scv_vector``'s rules:
    a scalar for the whole batch or a float64 ``[B]`` array.  A row gets
    ``(0, 0)`` when it breaks the row contract, its ``scv`` is invalid, its
    ``eps`` is no finite number in the open (0, 1), or its rate is NaN,
    infinite, <= 0 or above the rate range's maximum; ``Q_VALID`` tells such a
    row from a legitimate ``q = 0``.

    device: as in ``solve_problems``.  On ``cuda`` the rows with N <=
    GPU_MAX_BATCH_LIMIT (invalid rows ride along) run on the quantile kernel,
    one launch.  Rows with a larger N run on the native CPU solver while that
    launch runs, unless ``large_n`` is on: then those up to
    GPU_COMPACT_MAX_BATCH_LIMIT run on the compact quantile kernel
    (``submit_quantile_compact``, which keeps no table of the tail sum), one
    more launch enqueued before anything is collected, and only rows beyond
    that limit stay on the CPU.  Off the GPU: the torch-free binding, else the
    torch binding, else the Python analyzer.

    large_n: as in ``solve_problems``; ``None`` asks ``WVA_GPU_LARGE_N``.  No
    effect off the GPU, on rows with N <= GPU_MAX_BATCH_LIMIT, or under
    ``WVA_GPU_GRAPH=1``."""
    from . import get_native, get_native_cpu, native_available, native_cpu_available

    problems = np.ascontiguousarray(problems, dtype=np.float64)
    if problems.ndim != 2 or problems.shape[1] != PROBLEM_FIELDS:
        raise ValueError(f"problems must be [B, {PROBLEM_FIELDS}]")
    n_rows = problems.shape[0]
    rates = _scv_vector(rates, n_rows, "rates")
    eps = _scv_vector(eps, n_rows, "eps")
    scv_arr = None if scv is None else _scv_vector(scv, n_rows)
    if n_rows == 0:
        return np.zeros((0, QUANTILE_FIELDS), dtype=np.float64)

    if device is not None and str(device).startswith("cuda"):
        native = get_native()  # raises loudly if missing on a GPU box
        limits = _valid_batch_limits(problems)
        small = limits <= GPU_MAX_BATCH_LIMIT
        if small.all():
            with _on_device(device):
                return native.collect(native.submit_quantile(
                    problems, int(limits.max()), rates, eps, scv_arr))
        out = np.empty((n_rows, QUANTILE_FIELDS), dtype=np.float64)

        def part(mask):
            return (np.ascontiguousarray(problems[mask]), np.ascontiguousarray(rates[mask]),
                    np.ascontiguousarray(eps[mask]))

        def launch(submit, mask):
            with _on_device(device):
                return submit(part(mask)[0], int(limits[mask].max()), *part(mask)[1:],
                              None if scv_arr is None else np.ascontiguousarray(scv_arr[mask]))

        compact = ~small & (limits <= GPU_COMPACT_MAX_BATCH_LIMIT)
        if not _large_n_requested(large_n):
            compact[:] = False
        host = ~small & ~compact
        tickets = []
        if small.any():
            tickets.append((small, launch(native.submit_quantile, small)))
        try:
            if compact.any():
                tickets.append((compact, launch(native.submit_quantile_compact, compact)))
            if host.any():
                out[host] = ttft_quantiles(*part(host), device="cpu",
                                           scv=None if scv_arr is None else scv_arr[host])
        finally:  # a launch already enqueued must not keep its slot for good
            for mask, ticket in tickets:
                out[mask] = native.collect(ticket)
        return out

    if native_cpu_available():
        return get_native_cpu().ttft_quantiles(problems, rates, eps, scv_arr)
    if native_available():
        import torch

        return get_native().ttft_quantiles(
            torch.from_numpy(problems), torch.from_numpy(rates), torch.from_numpy(eps),
            None if scv_arr is None else torch.from_numpy(scv_arr),
        ).numpy()
    from . import warn_if_pure_python_fallback

    warn_if_pure_python_fallback()
    return _ttft_quantiles_python(
        problems, rates, eps, np.ones(n_rows) if scv_arr is None else scv_arr)


def itl_quantiles(problems: np.ndarray, rates, eps, device: Optional[str] = None,
                  large_n: Optional[bool] = None) -> np.ndarray:
    """The ITL that a share ``eps`` of each row's tokens exceeds at the
    per-replica rate ``rates`` (req/s): [B, 12] problems -> [B, 2] of ``(Q_VALID,
    Q_ITL)`` (csrc/queue_core.h, "ITL quantile"; ``QueueAnalyzer.itl_quantile``
    is the definition).  ``eps = 0.05`` asks for the p95 ITL in ms.

    ``rates`` and ``eps`` follow ``_scv_vector``'s rules: a scalar for the whole
    batch or a float64 ``[B]`` array.  There is no ``scv``: occupancy does not
    depend on the wait scale.  A row gets ``(0, 0)`` when it breaks the row
    contract, its ``eps`` is no finite number in the open (0, 1), or its rate is
    NaN, infinite, <= 0 or above the rate range's maximum.

    device: as in ``solve_problems``.  On ``cuda`` the rows with N <=
    GPU_MAX_BATCH_LIMIT (invalid rows ride along) run on the ITL quantile
    kernel, one ``submit_itl_quantile`` launch.  With ``large_n`` on, the rows up
    to GPU_COMPACT_MAX_BATCH_LIMIT take a second launch of the same kernel,
    which reserves LDS for them alone and is enqueued before anything is
    collected.  Every other row runs on the native CPU solver while the
    launches run.  Off the GPU: the torch-free binding, else the torch binding,
    else the Python analyzer.

    large_n: as in ``solve_problems``; ``None`` asks ``WVA_GPU_LARGE_N``.  No
    effect off the GPU, on rows with N <= GPU_MAX_BATCH_LIMIT, or under
    ``WVA_GPU_GRAPH=1``."""
    from . import get_native, get_native_cpu, native_available, native_cpu_available

    problems = np.ascontiguousarray(problems, dtype=np.float64)
    if problems.ndim != 2 or problems.shape[1] != PROBLEM_FIELDS:
        raise ValueError(f"problems must be [B, {PROBLEM_FIELDS}]")
    n_rows = problems.shape[0]
    rates = _scv_vector(rates, n_rows, "rates")
    eps = _scv_vector(eps, n_rows, "eps")
    if n_rows == 0:
        return np.zeros((0, QUANTILE_FIELDS), dtype=np.float64)

    if device is not None and str(device).startswith("cuda"):
        native = get_native()  # raises loudly if missing on a GPU box
        limits = _valid_batch_limits(problems)
        small = limits <= GPU_MAX_BATCH_LIMIT
        if small.all():
            with _on_device(device):
                return native.collect(native.submit_itl_quantile(
                    problems, int(limits.max()), rates, eps))
        middle = ~small & (limits <= GPU_COMPACT_MAX_BATCH_LIMIT)
        if not _large_n_requested(large_n):
            middle[:] = False
        host = ~small & ~middle
        out = np.empty((n_rows, QUANTILE_FIELDS), dtype=np.float64)
        tickets = []
        try:
            for mask in (small, middle):
                if mask.any():
                    rows, row_rates, row_eps = _masked(mask, problems, rates, eps)
                    with _on_device(device):
                        tickets.append((mask, native.submit_itl_quantile(
                            rows, int(limits[mask].max()), row_rates, row_eps)))
            if host.any():
                out[host] = itl_quantiles(*_masked(host, problems, rates, eps), device="cpu")
        finally:  # a launch already enqueued must not keep its slot for good
            for mask, ticket in tickets:
                out[mask] = native.collect(ticket)
        return out

    if native_cpu_available():
        return get_native_cpu().itl_quantiles(problems, rates, eps)
    if native_available():
        import torch

        return get_native().itl_quantiles(
            torch.from_numpy(problems), torch.from_numpy(rates), torch.from_numpy(eps)).numpy()
    from . import warn_if_pure_python_fallback

    warn_if_pure_python_fallback()
    return _itl_quantiles_python(problems, rates, eps)


def _resolved_scv(scv_rows, global_scv: float) -> np.ndarray:
    """The rows' cs^2 with the "use the fleet value" sentinel (any negative
    value) replaced by ``global_scv``: the vector a solver may see."""
    return np.array([s if s >= 0 else global_scv for s in scv_rows], dtype=np.float64)


class SyncDispatch:
    """submit/collect over today's synchronous ``solve_problems``: ``submit``
    solves on the spot and the ticket is the result.  Runs the chunked
    pipeline on any device.  ``global_scv`` is given when some server may
    need the M/G/1 correction: ``submit`` then resolves the rows' cs^2
    against it and passes the vector on, so the fleet is sized by the same
    native path as a Markovian one.  ``ttft_tail`` > 0 sizes every row to
    that TTFT tail probability (``solve_problems(..., ttft_tail=...)``), and
    ``itl_tail`` > 0 to that ITL tail fraction."""

    def __init__(self, device: Optional[str], global_scv: Optional[float] = None,
                 ttft_tail: float = 0.0, itl_tail: float = 0.0) -> None:
        self.device = device
        self.global_scv = global_scv
        self.ttft_tail = ttft_tail
        self.itl_tail = itl_tail

    def submit(self, problems: np.ndarray, scv_rows=None):
        extra = {"ttft_tail": self.ttft_tail} if self.ttft_tail > 0 else {}
        if self.itl_tail > 0:
            extra["itl_tail"] = self.itl_tail
        if self.global_scv is not None:
            scv_arr = _resolved_scv(scv_rows, self.global_scv)
            return solve_problems(problems, self.device, scv=scv_arr, **extra)
        return solve_problems(problems, self.device, **extra)

    def collect(self, ticket) -> np.ndarray:
        return ticket


class NativeGpuDispatch:
    """submit/collect over the native asynchronous dispatch
    (csrc/sizing_dispatch.h): ``submit`` returns once upload, kernel and
    download are enqueued, ``collect`` waits for them.  A chunk that needs
    the oversized-N split to the CPU is solved synchronously instead.
    ``global_scv`` is given when some server may need the M/G/1 correction:
    ``submit`` then resolves the rows' cs^2 against it and the vector travels
    with the rows, into the synchronous split too.  ``ttft_tail`` > 0 sizes
    every row to that TTFT tail probability: the rows with a TTFT target go
    to the waiting-time tail kernel as a second launch (``_TailTicket``) and
    the others through this class's own path, so the chunk stays
    asynchronous; a tail row above GPU_MAX_BATCH_LIMIT is solved on the CPU
    inside ``submit``.  ``itl_tail`` > 0 sizes every row's ITL target to that
    tail fraction: the rows with an ITL target go to the percentile kernel
    (``_PtileTicket``), enqueued first, and the others through this dispatch
    without it."""

    def __init__(self, native, device: str, global_scv: Optional[float] = None,
                 ttft_tail: float = 0.0, itl_tail: float = 0.0) -> None:
        self.native = native
        self.device = device
        self.global_scv = global_scv
        self.ttft_tail = self.itl_tail = 0.0
        # the mean-TTFT twin: this dispatch (of this class) without the tail,
        # for the rows of a split chunk that carry no TTFT target
        self._mean = copy.copy(self) if ttft_tail > 0 else None
        self.ttft_tail = ttft_tail
        # the mean-ITL twin: this dispatch without the ITL tail, for the rows
        # of a split chunk that carry no ITL target
        self._mean_itl = copy.copy(self) if itl_tail > 0 else None
        self.itl_tail = itl_tail

    def _submit_ptile(self, problems: np.ndarray, scv_rows, large_n: bool = False):
        """The chunk as a ``_PtileTicket``; its other rows go through the
        mean-ITL twin, TTFT tail included."""
        twin = self._mean_itl
        scv_arr = None
        if self.global_scv is not None:
            scv_arr = _resolved_scv(scv_rows, self.global_scv)
        n_rows = problems.shape[0]
        tail_arr = np.full(n_rows, self.ttft_tail) if self.ttft_tail > 0 else None
        return _PtileTicket(self.native, self.device, problems, np.full(n_rows, self.itl_tail),
                            tail_arr, scv_arr, lambda rows, scv, _tail: twin.submit(rows, scv),
                            twin.collect, large_n=large_n), None

    def _submit_split(self, problems: np.ndarray, scv_rows, large_n: bool = False):
        """The chunk as a ``_TailTicket``; its other rows go through the
        mean-TTFT twin (cs^2 values already resolved pass ``_resolved_scv``
        unchanged).  ``large_n``: whether a percentile row above
        GPU_MAX_BATCH_LIMIT goes to ``submit_tail_compact``, not to the CPU."""
        mean = self._mean
        scv_arr = None
        if self.global_scv is not None:
            scv_arr = _resolved_scv(scv_rows, self.global_scv)
        tail_arr = np.full(problems.shape[0], self.ttft_tail, dtype=np.float64)
        return _TailTicket(self.native, self.device, problems, tail_arr, scv_arr,
                           mean.submit, mean.collect, large_n=large_n), None

    def submit(self, problems: np.ndarray, scv_rows=None):
        if self.itl_tail > 0:
            return self._submit_ptile(problems, scv_rows)
        if self.ttft_tail > 0:
            return self._submit_split(problems, scv_rows)
        scv_arr = None
        if self.global_scv is not None:
            scv_arr = _resolved_scv(scv_rows, self.global_scv)
        max_batch = problems[:, P_MAX_BATCH].max()
        if not max_batch <= GPU_MAX_BATCH_LIMIT:  # also a NaN N
            if scv_arr is None:
                return None, solve_problems(problems, self.device)
            return None, solve_problems(problems, self.device, scv=scv_arr)
        max_k = max(int(max_batch), 1) * (1 + MAX_QUEUE_TO_BATCH_RATIO)
        with _on_device(self.device):
            if scv_arr is None:
                return self.native.submit(problems, max_k), None
            return self.native.submit(problems, max_k, scv_arr), None

    def collect(self, ticket) -> np.ndarray:
        native_ticket, solved = ticket
        if native_ticket is None:
            return solved
        if isinstance(native_ticket, (_TailTicket, _PtileTicket)):
            return native_ticket.collect()
        return self.native.collect(native_ticket)


class LargeNGpuDispatch(NativeGpuDispatch):
    """NativeGpuDispatch under the ``large_n`` opt-in (``solve_problems``):
    a chunk with a valid row above GPU_MAX_BATCH_LIMIT stays asynchronous, its
    rows up to GPU_COMPACT_MAX_BATCH_LIMIT going to the compact-table kernel
    as a second launch (``_LargeNTicket``).  Under ``ttft_tail`` > 0 the
    chunk's ``_TailTicket`` carries the opt-in: percentile rows up to
    GPU_COMPACT_MAX_BATCH_LIMIT go to the compact tail kernel
    (``submit_tail_compact``), so that chunk stays asynchronous too.  Any
    other chunk takes the parent class's path unchanged.
    ``BatchedAllocationSolver`` picks this class only when the opt-in is on,
    so the default pipeline runs the class above as it always did."""

    def submit(self, problems: np.ndarray, scv_rows=None):
        if self.itl_tail > 0:
            return self._submit_ptile(problems, scv_rows, large_n=True)
        if self.ttft_tail > 0:
            return self._submit_split(problems, scv_rows, large_n=True)
        if not problems[:, P_MAX_BATCH].max() <= GPU_MAX_BATCH_LIMIT:  # also a NaN N
            batch_limits = _valid_batch_limits(problems)
            if batch_limits.max() > GPU_MAX_BATCH_LIMIT:
                scv_arr = None
                if self.global_scv is not None:
                    scv_arr = _resolved_scv(scv_rows, self.global_scv)
                return _LargeNTicket(self.native, self.device, problems, batch_limits,
                                     scv_arr), None
            # only an invalid row has the large N: the parent class's path
        return super().submit(problems, scv_rows)

    def collect(self, ticket) -> np.ndarray:
        if isinstance(ticket[0], _LargeNTicket):
            return ticket[0].collect(self.native)
        return super().collect(ticket)


# Chunks the GPU pipeline splits a fleet into when the caller does not say
# (measured on the flagship shape: profiles/async_dispatch.md).
DEFAULT_GPU_CHUNKS = 2

# The launcher picks the chip-filling geometry from this many rows on
# (wva_launch_solve_scv); a fleet that could reach it is never chunked on the
# GPU, so every chunk runs the geometry the whole batch would have run.
_GPU_CHUNKING_ROW_BOUND = 512


class BatchedAllocationSolver:
    """Batched analyze phase: computes ``server.all_allocations`` for every
    server in a System through the native solver (semantically equal to
    ``System.calculate()``: same candidate order, batch size, cost and value
    bit for bit — tests/test_cycle_oracle.py).

    The servers are cut into ``chunks`` contiguous slices and driven as a
    pipeline over a submit/collect dispatch: build the rows of slice i,
    submit them, then collect slice i-1 and turn its results into
    Allocations.  On the GPU the host work of one slice overlaps the
    launch of another; results do not depend on the chunk count (rows are
    solved independently, and the GPU path chunks only while every chunk
    auto-selects the kernel geometry of the whole batch).  ``chunks=None``
    picks DEFAULT_GPU_CHUNKS on the GPU and 1 elsewhere; 1 is a single
    call.  A fleet in which some server may need the M/G/1 correction
    (``WVA_ANALYZER=mg1`` or a measured ``service_scv``) carries one cs^2 per
    row through the same dispatch; on the GPU it is chunked like any other
    fleet, elsewhere it is one chunk.  ``large_n`` is ``solve_problems``'
    opt-in for servers whose max batch exceeds GPU_MAX_BATCH_LIMIT: their
    rows run on the compact-table kernel and their chunk stays asynchronous
    (``None`` asks ``WVA_GPU_LARGE_N``; no effect off the GPU).
    ``ttft_percentile`` (in (0, 100), e.g. 95) sizes every server's TTFT
    target to that percentile of TTFT, not to its mean (module docstring,
    "TTFT percentile"); ``None`` asks ``WVA_TTFT_PERCENTILE``, read per call
    and unset by default, the knob ``core.create_allocation`` honours too.
    On the GPU those rows run on the waiting-time tail kernel and their chunk
    stays asynchronous; with ``large_n`` that holds for servers whose max
    batch exceeds GPU_MAX_BATCH_LIMIT too (the compact tail kernel).
    ``itl_percentile`` does the same for the ITL target (module docstring,
    "ITL percentile"); ``None`` asks ``WVA_ITL_PERCENTILE``.  On the GPU those
    rows run on the percentile kernel, which takes their TTFT percentile along.
    Under either knob the feasible allocations also carry the prediction at
    that percentile (``Allocation.ttft_percentile``, ``Allocation.itl_percentile``;
    the latter for servers with an ITL target), from one ``ttft_quantiles`` and
    one ``itl_quantiles`` call after the pipeline has drained, back to back.
    With both knobs unset no row list is kept and neither call is made.
    """

    def __init__(self, device: Optional[str] = None, chunks: Optional[int] = None,
                 large_n: Optional[bool] = None,
                 ttft_percentile: Optional[float] = None,
                 itl_percentile: Optional[float] = None) -> None:
        if chunks is not None and chunks < 1:
            raise ValueError("chunks must be at least 1")
        self.device = device
        self.chunks = chunks
        self.large_n = large_n
        self.ttft_tail = None if ttft_percentile is None else percentile_ttft_tail(ttft_percentile)
        self.itl_tail = None if itl_percentile is None else percentile_ttft_tail(itl_percentile)

    def _plan(self, system: System, servers):
        """The dispatch and chunk count for this fleet, decided before any
        submit; also whether rows must carry their server's cs^2."""
        from ..analyzer.mg1 import configured_scv

        global_scv = configured_scv()
        track_scv = global_scv != 1.0 or any(
            s >= 0 and s != 1.0 for s in [getattr(v, "service_scv", -1.0) for v in servers]
        )
        dispatch_scv = global_scv if track_scv else None
        tail = self.ttft_tail if self.ttft_tail is not None else configured_ttft_tail()
        itl = self.itl_tail if self.itl_tail is not None else configured_itl_tail()
        want_gpu = self.device is not None and str(self.device).startswith("cuda")
        if want_gpu and not _graph_requested():
            from . import get_native

            native = get_native()  # raises loudly if missing on a GPU box
            if native is None or not native.HAS_HIP:
                raise RuntimeError("the native HIP extension is required for device "
                                   f"{self.device!r} and is not built")
            chunks = self.chunks if self.chunks is not None else DEFAULT_GPU_CHUNKS
            if len(servers) * len(system.accelerators) >= _GPU_CHUNKING_ROW_BOUND:
                chunks = 1
            if _large_n_requested(self.large_n):
                return (LargeNGpuDispatch(native, self.device, dispatch_scv, tail, itl), chunks,
                        track_scv)
            return NativeGpuDispatch(native, self.device, dispatch_scv, tail, itl), chunks, track_scv
        if track_scv:
            return SyncDispatch(self.device, dispatch_scv, tail, itl), 1, True
        return SyncDispatch(self.device, ttft_tail=tail, itl_tail=itl), self.chunks or 1, False

    def _predict_percentiles(self, jobs, eps: float, global_scv: Optional[float]) -> None:
        """``ttft_percentile`` of every allocation in ``jobs``: its row at the
        per-replica rate ``create_allocation`` analyses, ``total_rate /
        num_replicas``, in one ``ttft_quantiles`` call (under the solver's
        ``large_n``, as the sizing was)."""
        problems = np.array([row for _, row, _ in jobs], dtype=np.float64)
        rates = problems[:, P_TOTAL_RATE] / np.array([a.num_replicas for a, _, _ in jobs],
                                                     dtype=np.float64)
        scv = None
        if global_scv is not None:
            scv = _resolved_scv([s for _, _, s in jobs], global_scv)
        solved = ttft_quantiles(problems, rates, eps, device=self.device, scv=scv,
                                large_n=self.large_n)
        for (alloc, _, _), (valid, q) in zip(jobs, solved.tolist()):
            if valid == 1.0:
                alloc.ttft_percentile = q

    def _predict_itl_percentiles(self, jobs, eps: float) -> None:
        """``itl_percentile`` of every allocation in ``jobs`` whose row has an
        ITL target (the rows the knob sized; ``create_allocation`` predicts for
        the same ones): one ``itl_quantiles`` call at ``_predict_percentiles``'
        rate and ``large_n``.  It runs after the TTFT prediction has been
        collected, back to back: the two share the job list, not the stream."""
        jobs = [job for job in jobs if job[1][P_TARGET_ITL] > 0]
        if not jobs:
            return
        problems = np.array([row for _, row, _ in jobs], dtype=np.float64)
        rates = problems[:, P_TOTAL_RATE] / np.array([a.num_replicas for a, _, _ in jobs],
                                                     dtype=np.float64)
        solved = itl_quantiles(problems, rates, eps, device=self.device, large_n=self.large_n)
        for (alloc, _, _), (valid, q) in zip(jobs, solved.tolist()):
            if valid == 1.0:
                alloc.itl_percentile = q

    def calculate(self, system: System) -> None:
        for g in system.accelerators.values():
            g.calculate()

        all_servers = list(system.servers.values())
        dispatch, n_chunks, track_scv = self._plan(system, all_servers)

        # pre-resolve the per-(model, accelerator) constants once — fleets
        # repeat model/accelerator combinations heavily
        pair_cache: Dict[Tuple[str, str], Optional[Tuple[float, float, float, float, int, int, float, int]]] = {}

        def pair_info(model, acc):
            key = (model.name, acc.name)
            hit = pair_cache.get(key, False)
            if hit is not False:
                return hit
            perf = model.get_perf_data(acc.name)
            if perf is None:
                pair_cache[key] = None
                return None
            info = (
                perf.decode_parms.alpha,
                perf.decode_parms.beta,
                perf.prefill_parms.gamma,
                perf.prefill_parms.delta,
                perf.max_batch_size,
                perf.at_tokens,
                acc.cost,
                model.get_num_instances(acc.name),
            )
            pair_cache[key] = info
            return info

        from ..core.allocation import sizing_headroom

        headroom_factor = 1.0 + sizing_headroom()
        accelerators = system.accelerators
        opt_spec = system.optimizer_spec
        energy_enabled = (
            opt_spec is not None
            and opt_spec.objective == "cost+energy"
            and opt_spec.energy_cost_per_kwh > 0
        )
        servers = system.servers
        # percentile sizing: every feasible allocation also gets its predicted
        # TTFT at that percentile, from one ttft_quantiles call after the
        # pipeline has drained, and under an ITL percentile its predicted ITL,
        # from one itl_quantiles call behind it: (allocation, row, its cs^2)
        eps, itl_eps = dispatch.ttft_tail, dispatch.itl_tail
        keep_rows = eps > 0 or itl_eps > 0
        quantile_jobs: List[Tuple[Allocation, Tuple[float, ...], float]] = []

        def build_rows(chunk_servers):
            """Build and submit the rows of one slice of servers; returns
            what apply_results needs once they are solved."""
            rows: List[Tuple[float, ...]] = []
            # (server, acc, N, unit cost, instances per replica)
            keys: List[Tuple[str, str, int, float, int]] = []
            zero_load: Dict[str, Dict[str, Allocation]] = {}
            scv_rows: List[float] = []  # per-server cs^2 (negative = use global)
            rows_append, keys_append = rows.append, keys.append
            scv_append = scv_rows.append

            for server in chunk_servers:
                server.all_allocations = {}
                load = server.load
                if (
                    load is None
                    or load.arrival_rate < 0
                    or load.avg_in_tokens < 0
                    or load.avg_out_tokens < 0
                ):
                    continue
                model = system.model(server.model_name)
                if model is None:
                    continue
                svc = system.service_class(server.service_class_name)
                if svc is None:
                    continue
                target = svc.model_target(server.model_name)
                if target is None:
                    continue
                target_ttft, target_itl, target_tps = target.ttft, target.itl, target.tps
                arrival, in_tok, out_tok = load.arrival_rate, load.avg_in_tokens, load.avg_out_tokens
                server_name = server.name
                server_max_batch = server.max_batch_size
                min_replicas = float(server.min_num_replicas)
                no_load = arrival == 0 or out_tok == 0
                if not no_load:
                    # the row fields that depend on the server alone, formed
                    # once for all its candidates
                    K = int(out_tok)
                    if K == 0 and server_max_batch > 0:
                        # 0 < out_tokens < 1: create_allocation's analyzer
                        # rejects the request size before TPS / K is formed
                        continue
                    in_tokens, out_tokens = float(int(in_tok)), float(K)
                    # (K == 0 without a batch override divides by zero in
                    # the N rule below, as create_allocation does)
                    total_rate = (
                        arrival / 60.0 if target_tps == 0 or K == 0 else target_tps / out_tokens
                    ) * headroom_factor
                candidates = server.get_candidate_accelerators(accelerators)
                for acc in candidates.values():
                    info = pair_info(model, acc)
                    if info is None:
                        continue
                    if no_load:
                        perf = model.get_perf_data(acc.name)
                        alloc = _zero_load_allocation(server, model, acc, perf)
                        zero_load.setdefault(server_name, {})[acc.name] = alloc
                        continue
                    alpha, beta, gamma, delta, perf_max_batch, at_tokens, unit_cost, instances = info
                    N = server_max_batch if server_max_batch > 0 else max(perf_max_batch * at_tokens // K, 1)
                    rows_append(
                        (alpha, beta, gamma, delta, in_tokens, out_tokens, float(N),
                         target_ttft, target_itl, target_tps, total_rate, min_replicas)
                    )
                    keys_append((server_name, acc.name, N, unit_cost, instances))
                    if track_scv:
                        scv_append(getattr(server, "service_scv", -1.0))

            ticket = None
            if rows:
                ticket = dispatch.submit(np.array(rows, dtype=np.float64), scv_rows)
            return ticket, keys, zero_load, (rows, scv_rows) if keep_rows else None

        def apply_results(ticket, keys, zero_load, submitted=None):
            """Collect one slice and turn its results into Allocations."""
            if ticket is not None:
                # plain floats beat numpy scalar access
                results_list = dispatch.collect(ticket).tolist()
            else:
                results_list = []
            for (server_name, acc_name, N, unit_cost, instances), res in zip(keys, results_list):
                if res[R_FEASIBLE] != 1.0:
                    continue
                server = servers[server_name]
                num_replicas = int(res[R_REPLICAS])
                alloc = Allocation(
                    accelerator=acc_name,
                    num_replicas=num_replicas,
                    batch_size=N,
                    # create_allocation's association: the product of the
                    # two integers is exact, so equal prices stay equal
                    cost=unit_cost * (instances * num_replicas),
                    itl=res[R_ITL],
                    ttft=res[R_TTFT],
                    rho=res[R_RHO],
                    max_arrv_rate_per_replica=res[R_RATE_STAR] / 1000.0,
                )
                cur = server.cur_allocation
                alloc.value = cur.transition_penalty(alloc) if cur is not None else alloc.cost
                if energy_enabled:
                    alloc.value += energy_value_term(system, server, alloc)
                server.all_allocations[acc_name] = alloc

            if submitted is not None:
                # a pass of its own, so that the loop above is what it is with
                # the knob unset; (server, accelerator) is unique among the keys
                rows, scv_rows = submitted
                for i, (key, res) in enumerate(zip(keys, results_list)):
                    if res[R_FEASIBLE] == 1.0:
                        alloc = servers[key[0]].all_allocations[key[1]]
                        quantile_jobs.append((alloc, rows[i], scv_rows[i] if scv_rows else -1.0))

            for server_name, accs in zero_load.items():
                server = servers[server_name]
                for acc_name, alloc in accs.items():
                    if server.cur_allocation is not None:
                        alloc.set_value(server.cur_allocation.transition_penalty(alloc))
                    if energy_enabled:
                        alloc.set_value(alloc.value + energy_value_term(system, server, alloc))
                    server.all_allocations[acc_name] = alloc

        # contiguous, near-equal slices of the servers; empty ones (more
        # chunks than servers) are skipped
        n = len(all_servers)
        bounds = [n * i // n_chunks for i in range(n_chunks + 1)]
        pending = None
        try:
            for lo, hi in zip(bounds, bounds[1:]):
                if lo == hi:
                    continue
                submitted = build_rows(all_servers[lo:hi])
                if pending is not None:
                    previous, pending = pending, submitted
                    apply_results(*previous)
                else:
                    pending = submitted
            if pending is not None:
                last, pending = pending, None
                apply_results(*last)
            if quantile_jobs and eps > 0:
                self._predict_percentiles(quantile_jobs, eps, dispatch.global_scv)
            if quantile_jobs and itl_eps > 0:
                self._predict_itl_percentiles(quantile_jobs, itl_eps)
        finally:
            # an exception between submit and collect must not leave a
            # launch uncollected (its slot would stay busy for good)
            if pending is not None and pending[0] is not None:
                try:
                    dispatch.collect(pending[0])
                except Exception:
                    pass

