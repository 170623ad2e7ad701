"""Percentile-TTFT rows with max batch 701..7680: the table-free tail sum
(Poisson recurrence over contiguous chunks) against the exact oracle.

Known-answer cases as in test_ops_ttft_tail, whose builders and bounds these
are: N in ``BATCH_LIMITS`` (701 the first routed N, 1024 a chunk edge, 7680
the LDS and Python limit), lam at 0.99 / 0.999 / 0.9999 of the rate range, t
at 0.5 / 3 oracle mean waits.  Of these 18 cells the two at N = 7680, f = 0.99
fall to the wait floor (the wait is 6e-12 of the service time).  Two more
cells at N = 701, f = 0.9999 clip the window: at 7.5 waits nu ~ 6214 of J =
7010 and ``hi`` stops at J - 1, at 8.5 waits nu ~ 7043 > J - 1 and the centre
itself is clipped.  The cell (7680, 0.999, 0.5) has nu ~ 38 and a window
shorter than 256 terms: some threads get an empty chunk.  The N <= 700 table
of test_ops_ttft_tail goes through the new entry points too, since small J
(N = 1, 2, 6, 7, 26) is where chunk arithmetic breaks.
"""

from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import ttft_tail_oracle as tail_oracle
from fixtures import make_system, server_spec
from test_ops_ttft_tail import BAD_EPS, FINAL_TOL, _case, _known, _row, arrays, check
from test_ops_ttft_tail import table as small_table
from wva_amd import ops
from wva_amd.ops import BatchedAllocationSolver, solve_problems
from wva_amd.ops import batched as B

BATCH_LIMITS = (701, 1024, 7680)
CPU = ops.get_native_cpu()
CPU_TAIL_COMPACT = CPU.solve_allocations_tail_compact  # absent before this kernel


@lru_cache(maxsize=None)
def table():
    cells = [_known(n, f, m) for n in BATCH_LIMITS for f in ("0.99", "0.999", "0.9999")
             for m in ("0.5", "3")]
    cases = [c for c in cells if c is not None]
    assert len(cells) - len(cases) <= len(cells) // 4, "too many cells dropped"
    assert {int(c["row"][B.P_MAX_BATCH]) for c in cases} == set(BATCH_LIMITS), "an N lost"
    cases += [_known(701, "0.9999", m) for m in ("7.5", "8.5")]  # the clipped window
    cases.append(_known(1024, "0.999", "3", scv=0.25))
    assert None not in cases
    for n in BATCH_LIMITS:
        row = _row(n)
        lam_min, lam_max = oracle.rate_range(row)
        top, bottom = oracle.evaluate(row, lam_max), oracle.evaluate(row, lam_min)
        # eps above y(lam_max): lam* = lam_max
        above = _row(n, float(2 * top.ttft))
        y_top = tail_oracle.ttft_exceedance(above, lam_max, above[B.P_TARGET_TTFT])
        cases.append(_case(above, (1 + y_top) / 2, lam_max, FINAL_TOL))
        # target_ttft <= prefill at every rate: P = 1 > eps
        cases.append(_case(_row(n, float((bottom.ttft - bottom.wait) / 2)), 0.05, None, None))
        # eps below y(lam_min): no float at these N (the oracle gives 1e-3437 at
        # N = 701 and less beyond), so the case cannot be written down; the
        # N <= 700 table, which the host reference and the kernel run too, has it
        below = _row(n, float(bottom.ttft - bottom.wait + 1 / oracle.model_of(row).mu[-1]))
        assert tail_oracle.ttft_exceedance(below, lam_min, below[B.P_TARGET_TTFT]) < 1e-320
    assert sum(c["lam"] is None for c in cases) == len(BATCH_LIMITS)
    assert sum(c["rate_tol"] == FINAL_TOL for c in cases) == len(BATCH_LIMITS)
    return cases


def _cpu(p, scv=None, eps=None):
    if eps is None:  # the same evaluator without the tail
        return CPU.solve_allocations_compact(p, scv)
    return CPU_TAIL_COMPACT(p, scv, eps)


def _torch(p, scv=None, eps=None):
    import torch

    native = ops.get_native()
    args = [torch.from_numpy(p)] + [None if v is None else torch.from_numpy(v) for v in (scv, eps)]
    if eps is None:
        return native.solve_allocations_compact(*args).numpy()
    return native.solve_allocations_tail_compact(*args).numpy()


def _kernel(p, scv=None, eps=None):
    native = ops.get_native()
    max_n = int(p[:, B.P_MAX_BATCH].max())
    if eps is None:
        return native.collect(native.submit_compact(p, max_n, scv))
    return native.collect(native.submit_tail_compact(p, max_n, eps, scv))


def _kernel_by_row(p, scv=None, eps=None):
    return np.concatenate([
        _kernel(p[i:i + 1], None if scv is None else scv[i:i + 1],
                None if eps is None else eps[i:i + 1]) for i in range(len(p))])


gpu = pytest.mark.gpu
# implementation, and the table it is held to
IMPLS = {
    "cpu_tail_compact": (_cpu, table),
    "cpu_tail_compact_small_n": (_cpu, small_table),
    "torch_tail_compact": (_torch, table),
    "kernel": (_kernel, table),
    "kernel_by_row": (_kernel_by_row, table),
    "kernel_small_n": (_kernel, small_table),
}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k.startswith("kernel") else k for k in IMPLS]


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_oracle_table(impl):
    solve, cases = IMPLS[impl]
    check(solve(*arrays(cases())), cases())


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_zero_vector_and_invalid_eps(impl):
    solve, cases = IMPLS[impl]
    p, scv, eps = arrays([c for c in cases() if c["rate_tol"] not in (None, FINAL_TOL)][::3])
    assert np.array_equal(solve(p, scv, np.zeros(len(p))), solve(p, scv)), "zero vector"
    # each invalid eps between two valid rows: a zero row, the others untouched
    valid = solve(p, scv, eps)
    mixed = np.tile(eps, len(BAD_EPS))
    mixed[1::len(p)] = BAD_EPS
    out = solve(np.tile(p, (len(BAD_EPS), 1)), np.tile(scv, len(BAD_EPS)), mixed)
    bad = np.zeros(len(mixed), dtype=bool)
    bad[1::len(p)] = True
    assert not out[bad].any()
    assert np.array_equal(out[~bad], np.tile(valid, (len(BAD_EPS), 1))[~bad])


@gpu
def test_solve_problems_routes_large_n_tail_rows():
    """eps = 0, eps > 0 at N <= 700, at N = 800 and at N = 8000, interleaved
    under large_n: each row from the route of its kind, back in its place."""
    known = [c for c in small_table() if c["rate_tol"] not in (None, FINAL_TOL)]
    mid, big = _known(800, "0.99", "3"), _known(8000, "0.999", "3")
    cases = [known[0], mid, known[-1], big, known[3], mid, known[-2]]
    p, scv, eps = arrays(cases)
    eps[[0, 4]] = 0.0
    calls = {"submit_tail": [], "submit_tail_compact": []}
    native = ops.get_native()
    with pytest.MonkeyPatch.context() as mp:
        for name, seen in calls.items():
            mp.setattr(native, name, lambda *a, _real=getattr(native, name), _seen=seen: (
                _seen.append(len(a[0])), _real(*a))[1])
        out = solve_problems(p, device="cuda", scv=scv, large_n=True, ttft_tail=eps)
    assert calls == {"submit_tail": [2], "submit_tail_compact": [2]}
    assert native.dispatch_pool_stats()[1] == 0
    check(out[[1, 2, 3, 5, 6]], [cases[i] for i in (1, 2, 3, 5, 6)])
    assert np.array_equal(out[[0, 4]], solve_problems(p[[0, 4]], device="cuda", scv=scv[[0, 4]]))
    assert np.array_equal(out[[1, 5]], _kernel(p[[1, 5]], scv[[1, 5]], eps[[1, 5]]))
    assert np.array_equal(out[[3]], CPU.solve_allocations(p[[3]], scv[[3]], eps[[3]]))
    # without the opt-in the N = 800 rows stay on the CPU solver
    off = solve_problems(p, device="cuda", scv=scv, large_n=False, ttft_tail=eps)
    assert np.array_equal(off[[1, 5]], CPU.solve_allocations(p[[1, 5]], scv[[1, 5]], eps[[1, 5]]))


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_large_n(device, monkeypatch):
    """Three servers with max batch 1024 under WVA_TTFT_PERCENTILE=95 and
    large_n: the batched solver agrees with System.calculate()."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=256, out_tokens=128,
                           max_batch=1024) for i, rate in enumerate((60000.0, 240000.0, 900000.0))]

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v.num_replicas
                for s in system.servers.values() for a, v in s.all_allocations.items()}

    monkeypatch.setenv("WVA_TTFT_PERCENTILE", "95")
    submits = []
    if device == "cuda":
        native = ops.get_native()
        monkeypatch.setattr(native, "submit_tail_compact", lambda *a, _real=native.submit_tail_compact: (
            submits.append(len(a[0])), _real(*a))[1])
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device, large_n=True).calculate)
    assert want and got == want
    assert bool(submits) == (device == "cuda")  # the rows ran on the compact tail kernel
    if device == "cuda":
        assert ops.get_native().dispatch_pool_stats()[1] == 0
