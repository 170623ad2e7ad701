"""The ITL quantile (``ops.itl_quantiles``) against the exact chain.

The reference: p[n+1] = p[n] lam / mu in 50-digit decimals, full
normalisation, no log space; tokens are emitted in proportion to p[n] mu(n),
``S_b`` is the share of the states with more than b requests in service (0 for
b = N), and ``b* = min{b in 1..N : S_b <= eps}``.  The answer is discrete, so a
case is usable only where eps is not within a relative 1e-6 of ``S_{b*-1}`` or
``S_{b*}``; the table is built so that every case is, and asserts it.  The value
must then be ``alpha + beta * b*`` within 2 ulp: one multiply and one add,
fused or not.

"The maximum" of the rate range is taken 1e-12 below it: its last bit depends
on whether a compiler fuses the multiply-adds of the service time, and a rate
one ulp above an implementation's own maximum is rejected, not solved.
"""

from decimal import Decimal as D, localcontext
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
from fixtures import make_system, server_spec
from wva_amd import ops
from wva_amd.ops import BatchedAllocationSolver
from wva_amd.ops import batched as B

BATCH_LIMITS = (1, 2, 63, 64, 65, 255, 256, 257, 700, 701, 7680)
FRACTIONS = (0.02, 0.6, 0.95, 1.0)
EPS = (0.5, 0.05, 0.001)
NAN, INF = float("nan"), float("inf")
gpu = pytest.mark.gpu


def _row(n, beta=None, in_tokens=512):
    if beta is None:  # a service rate that still rises at N
        beta = 0.027 if n <= 1000 else 0.0002
    row = np.zeros(12)
    row[:7] = (4.137, beta, 5.2, 0.0011, in_tokens, 128, n)
    row[B.P_TARGET_ITL], row[B.P_TOTAL_RATE], row[B.P_MIN_REPLICAS] = 20.0, 10.0, 1.0
    return row


def _top(row):
    return float(oracle.rate_range(row)[1] * 1000) * (1 - 1e-12)


@lru_cache(maxsize=None)
def _above(key, rate):
    """[b] = the unnormalised token mass of the states with more than b requests
    in service, b = 0..N ([0] is all of it, [N] is 0), in decimals."""
    m = oracle.model_of(np.array(key))
    with localcontext() as ctx:
        ctx.prec = 50
        p, weights = D(1), []
        for n in range(1, m.k + 1):
            mu = m.mu[min(n, m.n) - 1]
            p = p * D(rate) / 1000 / mu
            weights.append(p * mu)
        above, run = [D(0)] * (m.n + 1), D(0)
        for n in range(m.k, 0, -1):  # run: the states n and above
            run += weights[n - 1]
            if n <= m.n:
                above[n - 1] = run
        return above


def _case(n, frac, eps, **kw):
    case = case_of(_row(n, **kw), frac, eps)
    assert not case["tie"], (n, frac, eps)  # the honest-check condition; move the rate on a tie
    del case["tie"]
    return case


def case_of(row, frac, eps):
    """``_case`` on any valid row; ``tie``: eps within a relative 1e-6 of S_{b*-1} or S_{b*}."""
    n = int(row[B.P_MAX_BATCH])
    rate = _top(row) * frac
    above = _above(tuple(row), rate)
    with localcontext() as ctx:
        ctx.prec = 50
        cut = D(eps) * above[0]
        b = next(b for b in range(1, n + 1) if above[b] <= cut)
        tie = any(s != 0 and abs(cut / s - 1) <= D("1e-6") for s in (above[b - 1], above[b]))
    return {"row": row, "rate": rate, "eps": eps, "b": b, "tie": tie}


@lru_cache(maxsize=None)
def table():
    cases = [_case(n, f, e) for n in BATCH_LIMITS[:-1] for f in FRACTIONS for e in EPS]
    cases += [_case(7680, f, e) for f, e in ((0.02, 0.5), (0.95, 0.05), (1.0, 0.001))]
    cases += [_case(256, f, 0.05) for f in (0.4025, 0.409, 0.414)]  # b* = 63, 64, 65
    cases += [_case(700, 0.945, 0.001)]  # b* = 682, inside the last tile 640..700
    cases += [_case(64, 0.6, 0.05, beta=0.0), _case(64, 0.6, 0.05, in_tokens=0)]
    found = {(c["b"] == 1, c["b"] == int(c["row"][B.P_MAX_BATCH]))
             for c in cases if c["row"][B.P_MAX_BATCH] >= 2}
    assert found == {(True, False), (False, False), (False, True)}
    assert {63, 64, 65} <= {c["b"] for c in cases if c["row"][B.P_MAX_BATCH] > 65}, "tile edge"
    # the crossing (the state before b*) in the last tile of 64, and that tile partly filled
    assert any((c["b"] - 1) // 64 == n // 64 and (n + 1) % 64 and c["b"] < n
               for c in cases for n in [int(c["row"][B.P_MAX_BATCH])]), "last tile"
    return cases


def arrays(cases):
    return tuple(np.array([c[k] for c in cases]) for k in ("row", "rate", "eps"))


def _torch(p, rates, eps):
    import torch

    return ops.get_native().itl_quantiles(*map(torch.from_numpy, (p, rates, eps))).numpy()


def _kernel(p, rates, eps):
    native = ops.get_native()
    return native.collect(native.submit_itl_quantile(
        p, int(B._valid_batch_limits(p).max()), rates, eps))


IMPLS = {"python": B._itl_quantiles_python, "torch": _torch, "kernel": _kernel,
         "cpu": lambda *a: ops.get_native_cpu().itl_quantiles(*a)}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k == "kernel" else k for k in IMPLS]


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_oracle_table(impl):
    out = IMPLS[impl](*arrays(table()))
    assert out.shape == (len(table()), 2)
    for (valid, q), c in zip(out, table()):
        want = c["row"][B.P_ALPHA] + c["row"][B.P_BETA] * c["b"]
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], c["b"], q)
        assert valid == 1.0 and abs(q - want) <= 2 * np.spacing(want), what


@gpu
def test_kernel_rows_alone():
    p, rates, eps = arrays(table())
    batch = _kernel(p, rates, eps)
    for i in range(3, len(p), 17):
        assert np.array_equal(_kernel(p[i:i + 1], rates[i:i + 1], eps[i:i + 1]), batch[i:i + 1]), i


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_invalid_rows(impl):
    """Each rejected input between two valid rows: exactly (0, 0), and the
    valid rows bit-equal to their values without it."""
    solve = IMPLS[impl]
    first, second = [c for c in table() if c["eps"] == 0.05
                     and c["row"][B.P_MAX_BATCH] in (65, 257)][1::4][:2]
    bad = [dict(first, eps=e) for e in (0.0, 1.0, -0.1, NAN, INF, -INF)]
    bad += [dict(first, rate=r) for r in (0.0, -1.0, NAN, INF, 1.01 * _top(first["row"]))]
    bad += [dict(first, row=_row(0))]
    out = solve(*arrays([c for b in bad for c in (first, b, second)]))
    alone = solve(*arrays([first, second]))
    assert (alone[:, B.Q_VALID] == 1.0).all() and (alone[:, B.Q_ITL] > 0).all()
    assert not out[1::3].any()
    assert np.array_equal(out[0::3], np.tile(alone[:1], (len(bad), 1)))
    assert np.array_equal(out[2::3], np.tile(alone[1:], (len(bad), 1)))


@gpu
def test_launch_limits_and_routes():
    native = ops.get_native()
    cases = [c for c in table() if c["eps"] == 0.05]
    small = [c for c in cases if c["row"][B.P_MAX_BATCH] == 256][1:3]
    large = [c for c in cases if c["row"][B.P_MAX_BATCH] == 701][1:3]
    p, rates, eps = arrays(small + large)
    with pytest.raises(RuntimeError):
        native.submit_itl_quantile(p, 7873, rates, eps)
    assert native.dispatch_pool_stats()[1] == 0
    # a row above the launch's max_n: the zero row, the others untouched
    out = native.collect(native.submit_itl_quantile(p, 256, rates, eps))
    assert not out[2:].any() and np.array_equal(out[:2], _kernel(p[:2], rates[:2], eps[:2]))
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(native, "submit_itl_quantile", lambda *a, _real=native.submit_itl_quantile: (
            calls.append(int(a[1])), _real(*a))[1])
        out = ops.itl_quantiles(p, rates, eps, "cuda", large_n=True)
        host = ops.itl_quantiles(p, rates, eps, "cuda", large_n=False)
    assert calls == [256, 701, 256] and native.dispatch_pool_stats()[1] == 0
    assert np.array_equal(out, np.concatenate([_kernel(p[:2], rates[:2], eps[:2]),
                                               _kernel(p[2:], rates[2:], eps[2:])]))
    assert np.array_equal(host[:2], out[:2])
    assert np.array_equal(host[2:], IMPLS["cpu"](p[2:], rates[2:], eps[2:]))


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_knob(device, monkeypatch):
    """The ITL-tail test's five servers, one with N > 700: under
    WVA_ITL_PERCENTILE=95 every allocation carries its predicted p95 ITL, the
    same ``alpha + beta * b`` as System.calculate()'s; unset, nothing runs."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=16, out_tokens=128,
                           max_batch=n) for i, (rate, n) in enumerate(
                               ((2400.0, 8), (60000.0, 300), (90000.0, 512), (120000.0, 800),
                                (30000.0, 64)))]
    submits = []
    if device == "cuda":
        native = ops.get_native()
        monkeypatch.setattr(native, "submit_itl_quantile", lambda *a, _real=native.submit_itl_quantile: (
            submits.append(len(a[0])), _real(*a))[1])

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v for s in system.servers.values()
                for a, v in s.all_allocations.items()}

    unset = sized(BatchedAllocationSolver(device=device, large_n=True).calculate)
    assert unset and all(v.itl_percentile == 0.0 for v in unset.values()) and not submits
    monkeypatch.setenv("WVA_ITL_PERCENTILE", "95")
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device, large_n=True).calculate)
    assert want and set(got) == set(want)
    for key, alloc in got.items():
        assert alloc.itl_percentile == pytest.approx(want[key].itl_percentile, rel=1e-12), key
        assert alloc.itl_percentile >= alloc.itl, key
        assert alloc.clone().itl_percentile == alloc.itl_percentile
    assert any(v.itl_percentile > v.itl for v in got.values())
    assert (len(submits) > 0) == (device == "cuda")
