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
"""

from __future__ import annotations

import contextlib
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


def _scv_vector(scv, n_rows: int) -> np.ndarray:
    """An explicit ``scv`` — a scalar for the whole batch or a float64
    ``[B]`` array — as the C-contiguous float64 ``[B]`` vector the native
    bindings take.  An array of another dtype or shape raises, as the
    bindings do."""
    if isinstance(scv, np.ndarray) and scv.ndim > 0:
        if scv.dtype != np.float64:
            raise TypeError(f"scv must be float64, got {scv.dtype}")
        if scv.shape != (n_rows,):
            raise ValueError(f"scv must be a scalar or [B] = [{n_rows}], got {scv.shape}")
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


def _valid_batch_limits(problems: np.ndarray) -> np.ndarray:
    """Column N with the invalid rows' entries replaced by 1, so that they
    neither size a launch nor leave the GPU."""
    return np.where(valid_rows(problems), problems[:, P_MAX_BATCH], 1.0)


def _solve_problems_python(problems: np.ndarray, scv=1.0) -> np.ndarray:
    """Reference-semantics scalar fallback via the Python analyzer.

    ``scv`` is the service-time cs^2 — a scalar for the whole batch or a
    per-row float64 array (mg1 auto mode derives one per server); a row
    whose cs^2 fails ``valid_scv`` yields the all-zero row."""
    scv_arr = _scv_vector(scv, problems.shape[0])
    out = np.zeros((problems.shape[0], RESULT_FIELDS), dtype=np.float64)
    valid = valid_rows(problems) & valid_scv(scv_arr)
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
    large_n: Optional[bool] = None,
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
    GPU_MAX_BATCH_LIMIT, or under ``WVA_GPU_GRAPH=1``.
    """
    from . import get_native, native_available

    problems = np.ascontiguousarray(problems, dtype=np.float64)
    if problems.ndim != 2 or problems.shape[1] != PROBLEM_FIELDS:
        raise ValueError(f"problems must be [B, {PROBLEM_FIELDS}]")
    scv_arr = None if scv is None else _scv_vector(scv, problems.shape[0])
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
        return _solve_problems_python(problems, scv=scv)

    want_gpu = device is not None and str(device).startswith("cuda")
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
        if scv_arr is None:
            return get_native_cpu().solve_allocations(problems)
        return get_native_cpu().solve_allocations(problems, scv_arr)
    if native_available():
        import torch

        native = get_native()
        if scv_arr is None:
            return native.solve_allocations(torch.from_numpy(problems)).numpy()
        return native.solve_allocations(
            torch.from_numpy(problems), -1, torch.from_numpy(scv_arr)
        ).numpy()
    from . import warn_if_pure_python_fallback

    warn_if_pure_python_fallback()
    if scv_arr is None:
        return _solve_problems_python(problems)
    return _solve_problems_python(problems, scv=scv_arr)


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
    native path as a Markovian one."""

    def __init__(self, device: Optional[str], global_scv: Optional[float] = None) -> None:
        self.device = device
        self.global_scv = global_scv

    def submit(self, problems: np.ndarray, scv_rows=None):
        if self.global_scv is not None:
            scv_arr = _resolved_scv(scv_rows, self.global_scv)
            return solve_problems(problems, self.device, scv=scv_arr)
        return solve_problems(problems, self.device)

    def collect(self, ticket) -> np.ndarray:
        return ticket


class NativeGpuDispatch:
    """submit/collect over the native asynchronous dispatch
    (csrc/sizing_dispatch.h): ``submit`` returns once upload, kernel and
    download are enqueued, ``collect`` waits for them.  A chunk that needs
    the oversized-N split to the CPU is solved synchronously instead.
    ``global_scv`` is given when some server may need the M/G/1 correction:
    ``submit`` then resolves the rows' cs^2 against it and the vector travels
    with the rows, into the synchronous split too."""

    def __init__(self, native, device: str, global_scv: Optional[float] = None) -> None:
        self.native = native
        self.device = device
        self.global_scv = global_scv

    def submit(self, problems: np.ndarray, scv_rows=None):
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
        return self.native.collect(native_ticket)


class LargeNGpuDispatch(NativeGpuDispatch):
    """NativeGpuDispatch under the ``large_n`` opt-in (``solve_problems``):
    a chunk with a valid row above GPU_MAX_BATCH_LIMIT stays asynchronous, its
    rows up to GPU_COMPACT_MAX_BATCH_LIMIT going to the compact-table kernel
    as a second launch (``_LargeNTicket``).  Any other chunk takes the parent
    class's path unchanged.  ``BatchedAllocationSolver`` picks this class only
    when the opt-in is on, so the default pipeline runs the class above as it
    always did."""

    def submit(self, problems: np.ndarray, scv_rows=None):
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
    """

    def __init__(self, device: Optional[str] = None, chunks: Optional[int] = None,
                 large_n: Optional[bool] = None) -> None:
        if chunks is not None and chunks < 1:
            raise ValueError("chunks must be at least 1")
        self.device = device
        self.chunks = chunks
        self.large_n = large_n

    def _plan(self, system: System, servers):
        """The dispatch and chunk count for this fleet, decided before any
        submit; also whether rows must carry their server's cs^2."""
        from ..analyzer.mg1 import configured_scv

        global_scv = configured_scv()
        track_scv = global_scv != 1.0 or any(
            s >= 0 and s != 1.0 for s in [getattr(v, "service_scv", -1.0) for v in servers]
        )
        dispatch_scv = global_scv if track_scv else None
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
                return LargeNGpuDispatch(native, self.device, dispatch_scv), chunks, track_scv
            return NativeGpuDispatch(native, self.device, dispatch_scv), chunks, track_scv
        if track_scv:
            return SyncDispatch(self.device, dispatch_scv), 1, True
        return SyncDispatch(self.device), self.chunks or 1, False

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
            return ticket, keys, zero_load

        def apply_results(ticket, keys, zero_load):
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
        finally:
            # an exception between submit and collect must not leave a
            # launch uncollected (its slot would stay busy for good)
            if pending is not None and pending[0] is not None:
                try:
                    dispatch.collect(pending[0])
                except Exception:
                    pass

