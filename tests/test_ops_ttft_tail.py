"""Sizing to a TTFT percentile (``ttft_tail``) against the exact oracle.

Known-answer cases: at N in ``BATCH_LIMITS`` (J = 10 N is a partial wave at
N = 1, crosses one wave at 6 -> 7, the workgroup at 26; 700 is the LDS edge),
lam at 0.5 / 0.9 / 0.99 of the rate range and t at 0.5 / 3 oracle mean waits,
the row gets ``target_ttft = t + prefill`` and eps = the oracle's exceedance
there, so lam* is the chosen lam; the offered load puts the replica quotient
at m + 0.5.  ``rate_star`` must hold the project's bound ``2e-6 * cond +
1e-9``, cond from an oracle central difference; cells with cond > 100 are
dropped at construction, and so are cells whose oracle mean wait is below the
suite's wait floor (1e-4 of the service time, mm1k_oracle.WAIT_FLOOR): there
t is ~1e-10 of the prefill it is added to, y(lam) jumps to 1 within 1e-9 of
lam, so the central difference is no derivative, and where the wait is 0 the
exceedance is 1, which is no valid eps.  Both rules together drop 10 of 48
cells, within the 25 % cap asserted below.  Everything at a known lam
(lam_max) holds ``FINAL_TOL`` = 1e-11 of the benign table (test_ops_oracle).
"""

from decimal import Decimal as D
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import ttft_tail_oracle as tail_oracle
from fixtures import make_system, server_spec
from wva_amd import ops
from wva_amd.ops import BatchedAllocationSolver, solve_problems
from wva_amd.ops import batched as B

FINAL_TOL = 1e-11
BATCH_LIMITS = (1, 2, 6, 7, 26, 64, 256, 700)
ALPHA, GAMMA, DELTA = 4.137, 5.2, 0.0011  # test_ops_oracle's rows
_H = D("0.0001")
BAD_EPS = (float("nan"), float("inf"), -float("inf"), -0.1, 1.0, 1.5)


def _row(n, target_ttft=0.0):
    row = np.zeros(12)
    row[:8] = (ALPHA, 0.413 if n <= 6 else 0.027, GAMMA, DELTA, 512, 128, n, target_ttft)
    row[B.P_TOTAL_RATE], row[B.P_MIN_REPLICAS] = 10.0, 1.0
    return row


def _case(row, eps, lam, rate_tol, scv=1.0):
    """Expected results of ``row`` when lam* is ``lam`` (None: infeasible)."""
    case = {"row": row, "eps": float(eps), "scv": scv, "lam": lam, "rate_tol": rate_tol}
    if lam is not None:
        case["rate_star"] = oracle.evaluate(row, lam).throughput * 1000
        row[B.P_TOTAL_RATE] = float(D("3.5") * case["rate_star"])  # 4 replicas
        case["final"] = oracle.evaluate(row, D(float(row[B.P_TOTAL_RATE])) / 4 / 1000)
    return case


def _known(n, f, mult, scv=1.0):
    """The known-answer case of one cell, or None where it is dropped."""
    return known_of(_row(n), f, mult, scv)[0]


def known_of(row, f, mult, scv=1.0):
    """``_known`` on any valid row with no targets set (the row is written
    to): (case, None), or (None, the reason it is dropped)."""
    ws = (D(1) + D(scv)) / 2
    lam_min, lam_max = oracle.rate_range(row)
    lam = lam_min + D(f) * (lam_max - lam_min)
    at = oracle.evaluate(row, lam)
    if at.wait < oracle.WAIT_FLOOR * at.serv:
        return None, "wait_floor"
    row[B.P_TARGET_TTFT] = float(ws * D(mult) * at.wait + at.ttft - at.wait)

    def y(rate):
        return tail_oracle.ttft_exceedance(row, rate, row[B.P_TARGET_TTFT], ws)

    up, dn = lam * (1 + _H), lam * (1 - _H)
    slope_y = abs((y(up) - y(dn)) / y(lam))
    slope_thr = abs(oracle.evaluate(row, up).throughput - oracle.evaluate(row, dn).throughput)
    cond = float(slope_thr / at.throughput / slope_y) if slope_y else float("inf")
    if cond > 100:
        return None, "ill_conditioned"
    eps = y(lam)
    if not D("1e-280") < eps < 1:
        return None, "eps_out_of_range"
    return _case(row, eps, lam, 2e-6 * cond + 1e-9, scv), None


def _with_target(row, target_ttft):
    row = row.copy()
    row[B.P_TARGET_TTFT] = target_ttft
    return row


def no_search_of(row):
    """The cases of ``row`` (no targets set) that no search decides: lam* at the
    cap, and the one or two infeasible ones."""
    lam_min, lam_max = oracle.rate_range(row)
    top, bottom = oracle.evaluate(row, lam_max), oracle.evaluate(row, lam_min)
    # eps above y(lam_max): lam* = lam_max
    above = _with_target(row, float(2 * top.ttft))
    y_top = tail_oracle.ttft_exceedance(above, lam_max, above[B.P_TARGET_TTFT])
    cases = [_case(above, (1 + y_top) / 2, lam_max, FINAL_TOL)]
    # target_ttft <= prefill at every rate: P = 1 > eps (a decode-only row has no prefill)
    if bottom.ttft > bottom.wait:
        cases.append(_case(_with_target(row, float((bottom.ttft - bottom.wait) / 2)), 0.05, None, None))
    # eps below y(lam_min), where that is a float at all
    below = _with_target(row, float(bottom.ttft - bottom.wait + 1 / oracle.model_of(row).mu[-1]))
    y_bottom = tail_oracle.ttft_exceedance(below, lam_min, below[B.P_TARGET_TTFT])
    if y_bottom > D("1e-280"):
        cases.append(_case(below, y_bottom / 2, None, None))
    return cases


@lru_cache(maxsize=None)
def table():
    cells = [_known(n, f, m) for n in BATCH_LIMITS for f in ("0.5", "0.9", "0.99")
             for m in ("0.5", "3")]
    cases = [c for c in cells if c is not None]
    assert len(cells) - len(cases) <= len(cells) // 4, "too many cells dropped"
    assert {int(c["row"][B.P_MAX_BATCH]) for c in cases} == set(BATCH_LIMITS), "an N lost"
    cases.append(_known(64, "0.9", "3", scv=0.25))
    for n in BATCH_LIMITS:
        cases += no_search_of(_row(n))
    assert sum(c["lam"] is None for c in cases) > len(BATCH_LIMITS)
    return cases


def arrays(cases):
    return (np.array([c["row"] for c in cases]), np.array([c["scv"] for c in cases]),
            np.array([c["eps"] for c in cases]))


def check(out, cases):
    for res, c in zip(out, cases):
        what = (int(c["row"][B.P_MAX_BATCH]), c["eps"], c["scv"])
        if c["lam"] is None:
            assert not res.any(), what
            continue
        assert res[B.R_FEASIBLE] == 1.0 and res[B.R_REPLICAS] == 4.0, (what, res)
        assert abs(res[B.R_RATE_STAR] / float(c["rate_star"]) - 1) <= c["rate_tol"], (what, res)
        if c["rate_tol"] == FINAL_TOL:  # lam is known: so is the final rate
            fin, ws = c["final"], (1 + c["scv"]) / 2
            for got, want in ((res[B.R_ITL], fin.itl), (res[B.R_RHO], fin.rho),
                              (res[B.R_TTFT], fin.wait * D(ws) + fin.ttft - fin.wait)):
                assert abs(got / float(want) - 1) <= FINAL_TOL, (what, res)


def _torch(name):
    import torch

    def solve(p, scv=None, eps=None):
        t = [None if v is None else torch.from_numpy(v) for v in (scv, eps)]
        args = (torch.from_numpy(p), -1, *t) if name == "solve_allocations" else (
            torch.from_numpy(p), *t)
        return getattr(ops.get_native(), name)(*args).numpy()
    return solve


def _kernel(p, scv=None, eps=None):
    native = ops.get_native()
    max_n = int(p[:, B.P_MAX_BATCH].max())
    if eps is None:  # the same evaluator without the tail
        return native.collect(native.submit_compact(p, max_n, scv))
    return native.collect(native.submit_tail(p, max_n, eps, scv))


def _kernel_by_row(p, scv=None, eps=None):
    return np.concatenate([
        _kernel(p[i:i + 1], None if scv is None else scv[i:i + 1],
                None if eps is None else eps[i:i + 1]) for i in range(len(p))])


gpu = pytest.mark.gpu
IMPLS = {
    "python": lambda p, scv=None, eps=None: B._solve_problems_python(
        p, 1.0 if scv is None else scv, 0.0 if eps is None else eps),
    "cpu": lambda *a: ops.get_native_cpu().solve_allocations(*a),
    "cpu_compact": lambda *a: ops.get_native_cpu().solve_allocations_compact(*a),
    "torch": _torch("solve_allocations"),
    "torch_compact": _torch("solve_allocations_compact"),
    "kernel": _kernel,
    "kernel_by_row": _kernel_by_row,
}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k.startswith("kernel") else k for k in IMPLS]


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_oracle_table(impl):
    check(IMPLS[impl](*arrays(table())), table())


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_zero_vector_and_invalid_eps(impl):
    solve = IMPLS[impl]
    cases = [c for c in table() if c["rate_tol"] not in (None, FINAL_TOL)][::5]
    p, scv, eps = arrays(cases)
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
def test_solve_problems_merges_the_three_routes():
    """eps = 0, eps > 0 and N > 700 rows interleaved: every row comes back in
    its place, from the route of its kind."""
    known = [c for c in table() if c["rate_tol"] not in (None, FINAL_TOL)]
    big = _known(800, "0.99", "3")
    cases = [known[0], big, known[-1], known[3], big, known[-2]]
    p, scv, eps = arrays(cases)
    eps[[0, 3]] = 0.0
    calls = []
    native = ops.get_native()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(native, "submit_tail", lambda *a, _real=native.submit_tail: (
            calls.append(len(a[0])), _real(*a))[1])
        out = solve_problems(p, device="cuda", scv=scv, ttft_tail=eps)
    assert calls == [2] and native.dispatch_pool_stats()[1] == 0
    check(out[[1, 2, 4, 5]], [cases[i] for i in (1, 2, 4, 5)])
    assert np.array_equal(out[[0, 3]], solve_problems(p[[0, 3]], device="cuda", scv=scv[[0, 3]]))
    assert np.array_equal(out[[2, 5]], _kernel(p[[2, 5]], scv[[2, 5]], eps[[2, 5]]))
    assert np.array_equal(out[[1, 4]], IMPLS["cpu"](p[[1, 4]], scv[[1, 4]], eps[[1, 4]]))


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_knob(device, monkeypatch):
    """Three servers under WVA_TTFT_PERCENTILE=95: the batched solver agrees
    with System.calculate(), and the knob moves a replica count."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=256, out_tokens=128,
                           max_batch=n) for i, (rate, n) in enumerate(
                               ((2400.0, 8), (9000.0, 16), (30000.0, 64)))]

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v.num_replicas
                for s in system.servers.values() for a, v in s.all_allocations.items()}

    mean = sized(lambda s: s.calculate())
    monkeypatch.setenv("WVA_TTFT_PERCENTILE", "95")
    submits = []
    if device == "cuda":
        native = ops.get_native()
        monkeypatch.setattr(native, "submit_tail", lambda *a, _real=native.submit_tail: (
            submits.append(len(a[0])), _real(*a))[1])
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device).calculate)
    assert want and got == want
    assert any(want[k] > mean[k] for k in want), "p95 sizing never binds"
    assert bool(submits) == (device == "cuda")  # the tail rows ran on the tail kernel
    if device == "cuda":
        assert ops.get_native().dispatch_pool_stats()[1] == 0
