"""The TTFT quantile at max batch 701..7680: the compact quantile kernel
(``submit_quantile_compact``) and its host reference
(``ttft_quantiles_compact``) against the exact oracle.

Known answers as in ``test_ops_ttft_quantile``, whose builders and bound (``2e-6
* cond + 1e-9`` on t, ``FINAL_TOL`` where no search runs) these are.  N = 701 is
the first routed N, 1024 gives 10240 terms (a chunk edge) and 7680 is the LDS
limit; lam at 0.99 / 0.999 / 0.9999 of the rate range, t at 0.5 / 3 oracle mean
waits.  2 of the 18 cells drop (N = 7680 at 0.99: the wait floor), within the
25 % cap, and no N is lost.  (7680, 0.999, 0.5) has a window shorter than 64
terms, so lanes get empty chunks; (701, 0.9999, 7.5 / 8.5) clip the window at
J - 1 and then the centre itself.  The ``*_small_n`` runs take
``test_ops_ttft_quantile``'s table, where J = 10 N is below the 64 chunks.
"""

from decimal import Decimal as D
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import test_ops_ttft_quantile as Q
import ttft_tail_oracle as tail_oracle
from fixtures import make_system, server_spec
from test_ops_ttft_tail import BAD_EPS, FINAL_TOL, _row
from wva_amd import ops
from wva_amd.ops import BatchedAllocationSolver
from wva_amd.ops import batched as B

LARGE_N = (701, 1024, 7680)
NAN, INF = float("nan"), float("inf")


@lru_cache(maxsize=None)
def table():
    cells = [Q._known(n, f, m) for n in LARGE_N for f in ("0.99", "0.999", "0.9999")
             for m in ("0.5", "3")]
    cases = [c for c in cells if c is not None]
    assert len(cells) - len(cases) <= len(cells) // 4, "too many cells dropped"
    assert {int(c["row"][B.P_MAX_BATCH]) for c in cases} == set(LARGE_N), "an N lost"
    cases += [Q._known(701, "0.9999", "7.5"), Q._known(701, "0.9999", "8.5"),
              Q._known(1024, "0.999", "3", scv=0.25)]
    assert all(c is not None for c in cases)
    return cases + [Q._nobody_waits(n) for n in LARGE_N]


def _torch(p, rates, eps, scv):
    import torch

    return ops.get_native().ttft_quantiles_compact(
        *map(torch.from_numpy, (p, rates, eps, scv))).numpy()


def _kernel(p, rates, eps, scv):
    native = ops.get_native()
    max_n = min(int(B._valid_batch_limits(p).max()), B.GPU_COMPACT_MAX_BATCH_LIMIT)
    return native.collect(native.submit_quantile_compact(p, max_n, rates, eps, scv))


def _kernel_by_row(*a):
    return np.concatenate([_kernel(*(v[i:i + 1] for v in a)) for i in range(len(a[0]))])


gpu = pytest.mark.gpu
IMPLS = {
    "cpu_compact": lambda *a: ops.get_native_cpu().ttft_quantiles_compact(*a),
    "torch_compact": _torch,
    "kernel": _kernel,
    "kernel_by_row": _kernel_by_row,
}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k.startswith("kernel") else k for k in IMPLS]
TABLES = [(k, table) for k in IMPLS] + [("cpu_compact", Q.table), ("kernel", Q.table)]


@pytest.mark.parametrize("impl,cases", [
    pytest.param(k, t, marks=gpu if k.startswith("kernel") else (),
                 id=k + ("_small_n" if t is Q.table else "")) for k, t in TABLES])
def test_oracle_table(impl, cases):
    cases = cases()
    out = IMPLS[impl](*Q.arrays(cases))
    assert out.shape == (len(cases), 2)
    worst = 0.0
    for (valid, q), c in zip(out, cases):
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], c["scv"])
        assert valid == 1.0, what
        if c["tol"] is None:  # no search ran: q is the prefill time
            assert abs(q / c["prefill"] - 1) <= FINAL_TOL, (what, q)
            continue
        t_got = (q - c["prefill"]) / ((1 + c["scv"]) / 2)
        worst = max(worst, abs(t_got / c["t"] - 1) / c["tol"])
        assert abs(t_got - c["t"]) <= c["t"] * c["tol"], (what, t_got, c["t"], c["tol"])
    print(f"{impl}: worst oracle error / bound = {worst:.3g}")


# (N, fraction of the rate range, t in units of J / (20 mu_N)): eps of 1e-47 ...
# 1e-202 at a moderate load, where u = exp((J - i) d) underflows and
# quantile_sum_chunk leaves its chain for tail_sum_chunk's expm1 per term
SMALL_EPS_CELLS = ((701, "0.9", "3"), (701, "0.8", "3"), (1024, "0.85", "0.5"), (7680, "0.97", "3"))
CHAIN_MAX_EXPONENT, CHUNKS = 690.0, 64  # queue_core.h: kChainMaxExponent, kQuantileChunks


def chunks_on_fallback(case):
    """(chunks of the window at the case's t that take the expm1 fallback, the
    non-empty chunks), from the window rule stated in queue_core.h
    (tail_sweep_at) and the switch of quantile_sum_chunk."""
    m = oracle.model_of(case["row"])
    lam, mu_n, big_j = case["rate"] / 1000, float(m.mu[-1]), 10 * m.n
    d = np.log(lam) - np.log(mu_n)
    c = np.floor(min(lam * case["t"], big_j - 1))
    span = 37.54 + 2 * np.log(big_j)
    h = 2 * span + 1 + np.sqrt(2 * span * c)
    lo, hi = int(max(c - h, 0)), int(min(c + h, big_j - 1))
    length = (hi - lo + CHUNKS) // CHUNKS
    starts = [lo + part * length for part in range(CHUNKS) if lo + part * length <= hi]
    return sum((big_j - i0) * d < -CHAIN_MAX_EXPONENT for i0 in starts), len(starts)


@lru_cache(maxsize=None)
def small_eps_case(n, f, mult):
    """The known answer at t = mult J / (20 mu_N): Q._known with t given in
    service times, since the mean wait says nothing about a 1e-100 tail."""
    row, lam, at = Q._at(n, f)
    t = D(mult) * 10 * n / (20 * oracle.model_of(row).mu[-1])
    y, up, dn = (tail_oracle.exceedance(row, lam, t * s) for s in (1, 1 + Q._H, 1 - Q._H))
    cond = float(1 / abs((up - dn) / (2 * Q._H) / y))
    assert D("1e-280") < y < D("1e-40") and cond <= 100, (n, f, mult, y, cond)
    return {"row": row, "rate": float(lam * 1000), "eps": float(y), "scv": 1.0, "t": float(t),
            "prefill": float(at.ttft - at.wait), "tol": 2e-6 * cond + 1e-9}


@lru_cache(maxsize=None)
def small_eps_table():
    cases = [small_eps_case(*cell) for cell in SMALL_EPS_CELLS]
    # a later change of the window must not take the cases off the path they are for
    mixed, *rest = (chunks_on_fallback(c) for c in cases)
    assert 0 < mixed[0] < mixed[1], mixed  # chunks on each side of kChainMaxExponent
    assert all(fallback == chunks > 32 for fallback, chunks in rest), rest
    return cases


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_small_eps_takes_the_fallback_chunk(impl):
    """The expm1 fallback of quantile_sum_chunk, alone and mixed with the
    chain in one evaluation, holds the table's bound on t."""
    _check_t(impl, IMPLS[impl], small_eps_table())


@pytest.mark.parametrize("impl", [k if k in ("python", "cpu", "torch") else pytest.param(k, marks=gpu)
                                  for k in Q.IMPLS])
def test_small_eps_overlay(impl):
    """The N <= 700 analogue (N = 700, 0.9 of the rate range, t = 3 J / (20
    mu_N)) on the overlay quantile paths: no chain there, but no eps below 1e-3
    in their own table either."""
    _check_t(impl, Q.IMPLS[impl], [small_eps_case(700, "0.9", "3")])


def _check_t(impl, solve, cases):
    out = solve(*Q.arrays(cases))
    for (valid, q), c in zip(out, cases):
        t_got = (q - c["prefill"]) / ((1 + c["scv"]) / 2)
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], t_got, c["t"], c["tol"])
        print(f"{impl}: N = {what[0]}, eps = {c['eps']:.3g}: error / bound = "
              f"{abs(t_got / c['t'] - 1) / c['tol']:.3g}")
        assert valid == 1.0 and abs(t_got - c["t"]) <= c["t"] * c["tol"], what


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_rejected_inputs(impl):
    """Each rejected input between two valid N = 701 rows: exactly (0, 0), and
    the valid rows bit-equal to their values when solved alone.  The kernel
    also rejects a row whose N exceeds what the launch reserved."""
    solve = IMPLS[impl]
    first, second = [c for c in table() if c["tol"] is not None and c["scv"] == 1.0
                     and int(c["row"][B.P_MAX_BATCH]) == 701][:2]
    top = float(oracle.rate_range(first["row"])[1] * 1000)
    bad = [dict(first, eps=e) for e in BAD_EPS + (0.0,)]
    bad += [dict(first, rate=r) for r in (NAN, INF, -INF, 0.0, -1.0, 1.01 * top)]
    bad += [dict(first, scv=-0.5), dict(first, row=_row(0))]
    if impl.startswith("kernel"):  # N = 8000 in a launch with max_n = 7680
        bad.append(dict(first, row=_row(8000)))
    cases = [c for b in bad for c in (first, b, second)]
    out = solve(*Q.arrays(cases))
    alone = [solve(*Q.arrays([c])) for c in (first, second)]
    assert alone[0][0, 0] == 1.0 and alone[1][0, 0] == 1.0
    assert not out[1::3].any()
    assert np.array_equal(out[0::3], np.tile(alone[0], (len(bad), 1)))
    assert np.array_equal(out[2::3], np.tile(alone[1], (len(bad), 1)))


@gpu
def test_routing_splits_three_ways(monkeypatch):
    """N <= 700, N = 800 and N = 8000 rows interleaved: one launch per kernel
    with its rows alone, the N = 8000 row from the native CPU solver; with
    large_n off the N = 800 rows are the CPU solver's too."""
    small = [c for c in Q.table() if c["tol"] is not None][::7]

    def at(n):  # no oracle call: bit-equality alone is checked on these rows
        return {"row": _row(n), "rate": 0.9995 * float(oracle.rate_range(_row(n))[1] * 1000),
                "eps": 0.05, "scv": 1.0}

    cases = [small[0], at(800), at(8000), small[1], small[2], at(800)]
    p, rates, eps, scv = args = Q.arrays(cases)
    native, calls = ops.get_native(), []
    for name in ("submit_quantile", "submit_quantile_compact"):
        monkeypatch.setattr(native, name, lambda *a, _real=getattr(native, name), _n=name: (
            calls.append((_n, len(a[0]))), _real(*a))[1])
    out = ops.ttft_quantiles(p, rates, eps, device="cuda", scv=scv, large_n=True)
    assert calls == [("submit_quantile", 3), ("submit_quantile_compact", 2)]
    assert native.dispatch_pool_stats()[1] == 0
    cpu = ops.get_native_cpu().ttft_quantiles
    assert np.array_equal(out[[0, 3, 4]], Q._kernel(*(v[[0, 3, 4]] for v in args)))
    assert np.array_equal(out[[1, 5]], _kernel(*(v[[1, 5]] for v in args)))
    assert np.array_equal(out[[2]], cpu(*(v[[2]] for v in args)))
    assert (out[:, B.Q_VALID] == 1.0).all() and (out[[1, 2, 5], B.Q_TTFT] > 0).all()
    off = ops.ttft_quantiles(p, rates, eps, device="cuda", scv=scv, large_n=False)
    assert np.array_equal(off[[1, 2, 5]], cpu(*(v[[1, 2, 5]] for v in args)))
    assert np.array_equal(off[[0, 3, 4]], out[[0, 3, 4]])


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_prediction_large_n(device, monkeypatch):
    """test_fleet_percentile_large_n's servers under WVA_TTFT_PERCENTILE=95 and
    large_n: every allocation's predicted p95 TTFT equals System.calculate()'s
    (1e-4 guards the wiring), and on the GPU every row ran on the compact
    quantile kernel.  At the sized rates these servers run at a fifth of their
    batch, so under 5 % of the arrivals wait and no row searches: the search is
    the oracle table's job."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=256, out_tokens=128,
                           max_batch=1024) for i, rate in enumerate((60000.0, 240000.0, 900000.0))]
    submits = []
    if device == "cuda":
        native = ops.get_native()
        monkeypatch.setattr(native, "submit_quantile_compact",
                            lambda *a, _real=native.submit_quantile_compact: (
                                submits.append(len(a[0])), _real(*a))[1])

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v for s in system.servers.values()
                for a, v in s.all_allocations.items()}

    monkeypatch.setenv("WVA_TTFT_PERCENTILE", "95")
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device, large_n=True).calculate)
    assert want and set(got) == set(want)
    for key, alloc in got.items():
        assert alloc.ttft_percentile == pytest.approx(want[key].ttft_percentile, rel=1e-4), key
    assert all(v.ttft_percentile > 0 for v in got.values())
    assert submits == ([len(got)] if device == "cuda" else [])
