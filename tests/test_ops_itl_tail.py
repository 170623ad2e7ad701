"""Sizing to an ITL percentile (``itl_tail``) against the token-weighted
definition on the exact chain.

The reference, ``y_ref``: tokens are emitted in proportion to p[n] mu(n), p
from mm1k_oracle's recursion p[n+1] = p[n] lam / mu in 50-digit decimals with
the full normalisation; no arrival identity, no log space, no geometric tail.

Cases: ``target_itl = decode_time(c) + beta / 2`` for the wanted c, so nothing
ties.  Where the tail binds (0 < c < N), lam* comes from a float bisection of
the same definition, confirmed on ``y_ref`` to 1 % when the table is built; the
offered load is 3.5 lam*, so the replica quotient is never on an integer.  eps
lies a factor 10 inside (y(lam_min), y(lam_max)) in every binding cell but c =
1, eps = 0.001: y(lam_min) = 1 - pi_0 is 0.000999 there by the definition of
lam_min, a margin of 1e-3 where the search's tolerance is 1e-6.  The returned
``rate_star`` goes into ``y_ref`` and must give eps within 2e-6 eps, the
search's stop doubled (p[K] < 1e-13 at every binding lam*, asserted, so
throughput and arrival rate are the same number there).  Caps hold 1e-11.
"""

from decimal import Decimal as D, localcontext
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import ttft_tail_oracle as tail_oracle
from fixtures import make_system, server_spec
from wva_amd import ops
from wva_amd.analyzer import AnalyzerError, TargetPerf
from wva_amd.ops import BatchedAllocationSolver, solve_problems
from wva_amd.ops import batched as B

FINAL_TOL = 1e-11
BATCH_LIMITS = (1, 2, 63, 64, 65, 255, 256, 257, 700, 701, 7680)
BAD_EPS = (-0.1, 1.0, float("nan"), float("inf"), -float("inf"))
gpu = pytest.mark.gpu


def _weights(row, lam):
    """(token weight, decode time, p[K]) of the states 1..K, in decimals."""
    m = oracle.model_of(row)
    with localcontext() as ctx:
        ctx.prec = 50
        p, total, out = D(1), D(1), []
        for n in range(1, m.k + 1):
            b = min(n, m.n)
            p = p * D(lam) / m.mu[b - 1]
            total += p
            out.append((p * m.mu[b - 1], m.alpha + m.beta * b))
        return out, p / total


def y_ref(row, lam, target_itl):
    with localcontext() as ctx:
        ctx.prec = 50
        weights = _weights(row, lam)[0]
        return sum(w for w, t in weights if t > D(float(target_itl))) / sum(w for w, _ in weights)


def _y_float(row, lam, target_itl):
    """The same definition in float64, for placing lam* only."""
    m = oracle.model_of(row)
    b = np.minimum(np.arange(1, m.k + 1), m.n)
    mu = np.array([float(v) for v in m.mu])[b - 1]
    logw = np.cumsum(np.log(lam / mu)) + np.log(mu)
    w = np.exp(logw - logw.max())
    return w[row[B.P_ALPHA] + row[B.P_BETA] * b > target_itl].sum() / w.sum()


def _row(n, c, beta=None, in_tokens=512, target_ttft=0.0):
    if beta is None:  # a service rate that still rises at N: eps stays 10x under y(lam_max)
        beta = 0.027 if n <= 1000 else 0.0002
    row = np.zeros(12)
    row[:8] = (4.137, beta, 5.2, 0.0011, in_tokens, 128, n, target_ttft)
    row[B.P_TARGET_ITL] = 4.137 + beta * c + beta / 2 if beta else 4.137 * (1.5 if c else 0.5)
    row[B.P_TOTAL_RATE], row[B.P_MIN_REPLICAS] = 10.0, 1.0
    return row


def _case(row, c, eps, scv=1.0, ttft_eps=0.0, inside=10):
    n = int(row[B.P_MAX_BATCH])
    lam_min, lam_max = (float(v) for v in oracle.rate_range(row))
    case = {"row": row, "eps": eps, "scv": scv, "ttft_eps": ttft_eps, "kind": "cap", "lam": lam_max}
    if c == 0:
        return dict(case, kind="infeasible")
    if c < n:
        lo, broken = binding_lam(row, eps, inside, (c, eps) == (1, 0.001))
        assert broken is None, (n, c, eps, broken)
        case.update(kind="itl", lam=lo)
    row[B.P_TOTAL_RATE] = 3.5 * float(oracle.evaluate(row, case["lam"]).throughput) * 1000
    return case


def eps_range(row):
    """(y(lam_min), y(lam_max)) of the row's ITL target, in floats."""
    lam_min, lam_max = (float(v) for v in oracle.rate_range(row))
    target = row[B.P_TARGET_ITL]
    return _y_float(row, lam_min, target), _y_float(row, lam_max, target)


def binding_lam(row, eps, inside=10, near_bottom=False):
    """(lam* of a binding ITL tail, None), or (None, the rule of ``_case`` that
    the row breaks)."""
    lam_min, lam_max = (float(v) for v in oracle.rate_range(row))
    target = row[B.P_TARGET_ITL]
    y0, y1 = eps_range(row)
    if not (y0 * (1 + 1e-4) < eps < y1 / inside and (10 * y0 <= eps or near_bottom)):
        return None, "eps_near_range_end"
    lo, hi = lam_min, lam_max
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _y_float(row, mid, target) < eps else (lo, mid)
    if not abs(float(y_ref(row, lo, target)) / eps - 1) < 1e-2:
        return None, "placement_off"
    if not _weights(row, lo)[1] < D("1e-13"):
        return None, "blocking"
    return lo, None


@lru_cache(maxsize=None)
def table():
    cases = [_case(_row(n, c), c, eps) for n in BATCH_LIMITS for c in sorted({0, 1, n - 1, n})
             for eps in (0.05, 0.001)]
    cases += [_case(_row(64, c, in_tokens=0), c, 0.05) for c in (0, 63, 64)]  # decode-only
    cases += [_case(_row(64, c, beta=0.0), c, 0.05) for c in (0, 64)]
    assert sum(c["kind"] == "itl" for c in cases) >= 2 * len(BATCH_LIMITS)
    return cases


def _mixed_case(n, c, ttft_binds):
    """scv = 4 and ttft_tail = 0.05 on the same row.  P(W > t) <= P(n >= N) <=
    y_itl, so the TTFT tail can bind first only under a larger itl_tail: 0.3
    there, with the TTFT target the p95 TTFT at 0.97 of the ITL search's lam*.
    The other rows keep itl_tail = 0.05 and get a TTFT target ten times the
    mean TTFT at lam*, which the check confirms is the looser one."""
    # (itl_tail = 0.3 is where the ITL search is not meant to bind: a factor 3 will do)
    case = _case(_row(n, c), c, 0.3 if ttft_binds else 0.05, scv=4.0, ttft_eps=0.05,
                 inside=3 if ttft_binds else 10)
    row, ws = case["row"], D("2.5")
    if not ttft_binds:
        row[B.P_TARGET_TTFT] = 10 * float(oracle.evaluate(row, case["lam"]).ttft)
        return case
    lam = 0.97 * case["lam"]
    at = oracle.evaluate(row, lam)
    lo, hi = at.ttft - at.wait, at.ttft + 200 * at.wait + 10
    for _ in range(45):  # the TTFT whose exceedance at lam is 0.05
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if tail_oracle.ttft_exceedance(row, lam, mid, ws) > D("0.05") else (lo, mid)
    assert lo > (at.ttft - at.wait) * (1 + D("1e-3")), "nobody waits at this rate"
    row[B.P_TARGET_TTFT] = float(lo)
    row[B.P_TOTAL_RATE] = 3.5 * float(at.throughput) * 1000
    return dict(case, kind="ttft", lam=lam)


@lru_cache(maxsize=None)
def mixed_table():
    return [_mixed_case(64, 63, True), _mixed_case(256, 255, True), _mixed_case(64, 63, False),
            _mixed_case(701, 700, False)]


def arrays(cases):
    return (np.array([c["row"] for c in cases]), np.array([c["scv"] for c in cases]),
            np.array([c["ttft_eps"] for c in cases]), np.array([c["eps"] for c in cases]))


def check(out, cases, mean_solve):
    """``mean_solve``: the same solver without any tail, for the final fields."""
    p, scv = arrays(cases)[:2]
    finals = p.copy()
    finals[:, B.P_TARGET_TTFT:B.P_TARGET_TPS + 1] = 0.0
    finals[:, B.P_MIN_REPLICAS] = 4.0
    finals = mean_solve(finals, scv)
    for res, fin, c in zip(out, finals, cases):
        row, what = c["row"], (int(c["row"][B.P_MAX_BATCH]), c["kind"], c["eps"], res)
        if c["kind"] == "infeasible":
            assert not res.any(), what
            continue
        assert res[B.R_FEASIBLE] == 1.0 and res[B.R_REPLICAS] == 4.0, what
        lam = res[B.R_RATE_STAR] / 1000
        y_itl = float(y_ref(row, lam, row[B.P_TARGET_ITL])) if c["kind"] != "cap" else 0.0
        if c["kind"] == "itl":
            assert abs(y_itl - c["eps"]) <= 2e-6 * c["eps"], (what, y_itl / c["eps"] - 1)
        elif c["kind"] == "ttft":
            y = float(tail_oracle.ttft_exceedance(row, lam, row[B.P_TARGET_TTFT], D("2.5")))
            assert abs(y - c["ttft_eps"]) <= 2e-6 * c["ttft_eps"] and y_itl < c["eps"], what
        else:
            want = float(oracle.evaluate(row, c["lam"]).throughput) * 1000
            # a wide-range row carries its own bound (test_ops_percentile_wide)
            assert abs(res[B.R_RATE_STAR] / want - 1) <= c.get("final_tol", FINAL_TOL), what
        if c["kind"] == "itl" and c["ttft_eps"] > 0:  # the TTFT tail is the looser one
            assert tail_oracle.ttft_exceedance(row, lam, row[B.P_TARGET_TTFT], D("2.5")) < D("0.05")
        np.testing.assert_allclose(res[B.R_ITL:], fin[B.R_ITL:], rtol=FINAL_TOL, err_msg=str(what))


def _opt(v):
    return None if v is None or not np.any(v) else v


def _python(p, scv=None, tt=None, itl=None):
    return B._solve_problems_python(p, 1.0 if scv is None else scv, 0.0 if tt is None else tt,
                                    0.0 if itl is None else itl)


def _cpu(p, scv=None, tt=None, itl=None):
    return ops.get_native_cpu().solve_allocations_ptile(p, scv, tt, itl)


def _torch(p, scv=None, tt=None, itl=None):
    import torch

    return ops.get_native().solve_allocations_ptile(
        torch.from_numpy(p), *(None if v is None else torch.from_numpy(v) for v in (scv, tt, itl))
    ).numpy()


def _kernel(p, scv=None, tt=None, itl=None, split=False):
    native = ops.get_native()
    max_n = int(p[:, B.P_MAX_BATCH].max())
    if itl is None:  # the same evaluators without the occupancy tail
        submit = native.submit_compact if _opt(tt) is None else native.submit_tail_compact
        return native.collect(submit(p, max_n, *(() if _opt(tt) is None else (tt,)), scv))
    return native.collect(native.submit_ptile(p, max_n, itl, tt, scv, split))


def _kernel_by_row(p, *vecs):
    return np.concatenate([_kernel(p[i:i + 1], *(None if v is None else v[i:i + 1] for v in vecs))
                           for i in range(len(p))])


IMPLS = {"python": _python, "cpu": _cpu, "torch": _torch, "kernel": _kernel}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k == "kernel" else k for k in IMPLS]
# the measured alternative arrangement (submit_ptile(split=True)): same answers
IMPLS["kernel_split"] = lambda p, scv=None, tt=None, itl=None: _kernel(p, scv, tt, itl, itl is not None)
WITH_SPLIT = IMPL_PARAMS + [pytest.param("kernel_split", marks=gpu)]


@pytest.mark.parametrize("impl", WITH_SPLIT)
def test_oracle_table(impl):
    check(IMPLS[impl](*arrays(table())), table(), IMPLS[impl])


@pytest.mark.parametrize("impl", WITH_SPLIT)
def test_with_scv_and_ttft_tail(impl):
    check(IMPLS[impl](*arrays(mixed_table())), mixed_table(), IMPLS[impl])


@gpu
def test_kernel_rows_alone():
    cases = table()[3::9] + mixed_table()[:2]
    check(_kernel_by_row(*arrays(cases)), cases, _kernel)


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_zero_vector_and_invalid_eps(impl):
    solve = IMPLS[impl]
    cases = [c for c in table() if c["kind"] == "itl"][::7] + mixed_table()[:2]
    p, scv, tt, itl = arrays(cases)
    # the solve without the vector: the entry point the same binding had before
    parent = {"python": _python, "kernel": _kernel, "torch": _torch_parent,
              "cpu": lambda *a: ops.get_native_cpu().solve_allocations_tail_compact(*a)}[impl]
    assert np.array_equal(solve(p, scv, tt, np.zeros(len(p))), parent(p, scv, tt)), "zero vector"
    assert np.array_equal(solve(p, scv, tt, None), parent(p, scv, tt)), "no vector"
    # target_itl = 0 ignores a valid eps, inside every implementation
    no_itl = p.copy()
    no_itl[:, B.P_TARGET_ITL] = 0.0
    assert np.array_equal(solve(no_itl, scv, tt, itl), parent(no_itl, scv, tt)), "no ITL target"
    # each invalid eps between two valid rows: a zero row, the others untouched
    valid = solve(p, scv, tt, itl)
    k = len(BAD_EPS)
    mixed = np.tile(itl, k)
    mixed[1::len(p)] = BAD_EPS
    out = solve(np.tile(p, (k, 1)), np.tile(scv, k), np.tile(tt, k), mixed)
    bad = np.zeros(len(mixed), dtype=bool)
    bad[1::len(p)] = True
    assert not out[bad].any()
    assert np.array_equal(out[~bad], np.tile(valid, (k, 1))[~bad])


def _torch_parent(p, scv, tt):
    import torch

    return ops.get_native().solve_allocations_tail_compact(
        torch.from_numpy(p), torch.from_numpy(scv), torch.from_numpy(tt)).numpy()


def test_analyzer_contract():
    with pytest.raises(AnalyzerError):
        TargetPerf(target_itl=10.0, itl_tail=1.0).check()
    case = next(c for c in table() if c["kind"] == "itl" and c["row"][B.P_MAX_BATCH] == 64)
    row = case["row"].copy()
    row[B.P_TARGET_ITL] = 0.0  # no ITL target: a valid eps is ignored
    itl = np.array([case["eps"]])
    assert np.array_equal(solve_problems(row[None], "cpu", itl_tail=itl), solve_problems(row[None], "cpu"))


@gpu
def test_launch_limits_and_routes():
    native = ops.get_native()
    cases = [c for c in table() if c["kind"] == "itl" and c["eps"] == 0.05]
    small = [c for c in cases if c["row"][B.P_MAX_BATCH] == 256][:2]
    large = [c for c in cases if c["row"][B.P_MAX_BATCH] == 701][:2]
    p, scv, tt, itl = arrays(small + large)
    with pytest.raises(RuntimeError):
        native.submit_ptile(p, 7873, itl)
    assert native.dispatch_pool_stats()[1] == 0
    # a row above the launch's max_n: the all-zero row, the others untouched
    out = native.collect(native.submit_ptile(p, 256, itl))
    assert not out[2:].any() and np.array_equal(out[:2], _kernel(p[:2], None, None, itl[:2]))
    # routing: eps = 0 rows on today's launches, bit for bit, the others on submit_ptile
    itl[[0, 2]] = 0.0
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(native, "submit_ptile", lambda *a, _real=native.submit_ptile: (
            calls.append(int(a[1])), _real(*a))[1])
        out = solve_problems(p, "cuda", large_n=True, itl_tail=itl)
        host = solve_problems(p, "cuda", large_n=False, itl_tail=itl)
        assert np.array_equal(solve_problems(p, "cuda", large_n=True, itl_tail=np.zeros(4)),
                              solve_problems(p, "cuda", large_n=True))
    assert calls == [256, 701, 256] and native.dispatch_pool_stats()[1] == 0
    assert np.array_equal(out[[0, 2]], solve_problems(p[[0, 2]], "cuda", large_n=True))
    assert np.array_equal(out[[1, 3]], _kernel_by_row(p[[1, 3]], None, None, itl[[1, 3]]))
    assert np.array_equal(host[3:], _cpu(p[3:], None, None, itl[3:]))


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_knob(device, monkeypatch):
    """Five servers, one with N > 700, under WVA_ITL_PERCENTILE=95: the batched
    solver agrees with System.calculate(), and the knob moves a replica count."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=16, out_tokens=128,
                           max_batch=n) for i, (rate, n) in enumerate(
                               ((2400.0, 8), (60000.0, 300), (90000.0, 512), (120000.0, 800),
                                (30000.0, 64)))]

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v.num_replicas
                for s in system.servers.values() for a, v in s.all_allocations.items()}

    mean = sized(lambda s: s.calculate())
    assert sized(BatchedAllocationSolver(device=device, large_n=True).calculate) == mean
    monkeypatch.setenv("WVA_ITL_PERCENTILE", "95")
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device, large_n=True).calculate)
    assert want and got == want
    assert got == sized(BatchedAllocationSolver(device=device, large_n=True, itl_percentile=95,
                                                chunks=1).calculate)
    assert any(want[k] != mean[k] for k in set(want) & set(mean)), "p95 ITL sizing never binds"
    if device == "cuda":
        assert ops.get_native().dispatch_pool_stats()[1] == 0
