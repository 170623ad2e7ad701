"""The TTFT quantile (``ops.ttft_quantiles``) against the exact oracle.

Known answers: ``test_ops_ttft_tail``'s rows at its N (J = 10 N is a partial
wave at N = 1, crosses one wave at 6 -> 7, the workgroup at 26; 700 is the LDS
edge), lam at 0.5 / 0.9 / 0.99 of the rate range and t at 0.5 / 3 oracle mean
waits.  eps is the oracle's P(W > t) there, so the answer is ``q = ws * t +
prefill``.  The bound on t is the project's ``2e-6 * cond + 1e-9`` (the search
stops at 1e-6 relative on y, twice that for the two sides of the stop), with
cond = |y / (t y'(t))| from an oracle central difference in t (h = 1e-4).
Cells with cond > 100 or an oracle mean wait below the suite's wait floor are
dropped at construction: 11 of 48, within the 25 % cap asserted below, and no
N is lost.  Where no search runs (nobody waits that often) q is the prefill
time and holds ``FINAL_TOL`` = 1e-11.
"""

from decimal import Decimal as D
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import ttft_tail_oracle as tail_oracle
from fixtures import make_system, server_spec
from test_ops_ttft_tail import BAD_EPS, BATCH_LIMITS, FINAL_TOL, _row
from wva_amd import ops
from wva_amd.ops import BatchedAllocationSolver
from wva_amd.ops import batched as B

_H = D("0.0001")
NAN, INF = float("nan"), float("inf")


def _at(n, f):
    return at_of(_row(n), f)


def at_of(row, f):
    lam_min, lam_max = oracle.rate_range(row)
    lam = lam_min + D(f) * (lam_max - lam_min)
    return row, lam, oracle.evaluate(row, lam)


def _known(n, f, mult, scv=1.0):
    """The known-answer case of one cell, or None where it is dropped."""
    return known_of(_row(n), f, mult, scv)[0]


def known_of(row, f, mult, scv=1.0):
    """``_known`` on any valid row: (case, None), or (None, the reason it is
    dropped)."""
    row, lam, at = at_of(row, f)
    if at.wait < oracle.WAIT_FLOOR * at.serv:
        return None, "wait_floor"
    t = D(mult) * at.wait
    y, up, dn = (tail_oracle.exceedance(row, lam, t * s) for s in (1, 1 + _H, 1 - _H))
    if not D("1e-280") < y < 1:
        return None, "eps_out_of_range"
    slope = abs((up - dn) / (2 * _H) / y)  # |t y'(t) / y|
    if not slope or 1 / slope > 100:
        return None, "ill_conditioned"
    return {"row": row, "rate": float(lam * 1000), "eps": float(y), "scv": scv, "t": float(t),
            "prefill": float(at.ttft - at.wait), "tol": 2e-6 * float(1 / slope) + 1e-9}, None


def _nobody_waits(n):
    return nobody_waits_of(_row(n))


def nobody_waits_of(row, f="0.5", scv=1.0):
    row, lam, at = at_of(row, f)
    p_wait = tail_oracle.exceedance(row, lam, D("1e-30"))
    return {"row": row, "rate": float(lam * 1000), "eps": float((1 + p_wait) / 2), "scv": scv,
            "t": 0.0, "prefill": float(at.ttft - at.wait), "tol": None}


@lru_cache(maxsize=None)
def table():
    cells = [_known(n, f, m) for n in BATCH_LIMITS for f in ("0.5", "0.9", "0.99")
             for m in ("0.5", "3")]
    cases = [c for c in cells if c is not None]
    assert len(cells) - len(cases) <= len(cells) // 4, "too many cells dropped"
    assert {int(c["row"][B.P_MAX_BATCH]) for c in cases} == set(BATCH_LIMITS), "an N lost"
    cases.append(_known(64, "0.9", "3", scv=0.25))
    return cases + [_nobody_waits(n) for n in BATCH_LIMITS]


def arrays(cases):
    return tuple(np.array([c[k] for c in cases]) for k in ("row", "rate", "eps", "scv"))


def _torch(p, rates, eps, scv):
    import torch

    return ops.get_native().ttft_quantiles(*map(torch.from_numpy, (p, rates, eps, scv))).numpy()


def _kernel(p, rates, eps, scv):
    native = ops.get_native()
    max_n = int(B._valid_batch_limits(p).max())
    return native.collect(native.submit_quantile(p, max_n, rates, eps, scv))


def _kernel_by_row(*a):
    return np.concatenate([_kernel(*(v[i:i + 1] for v in a)) for i in range(len(a[0]))])


gpu = pytest.mark.gpu
IMPLS = {
    "python": B._ttft_quantiles_python,
    "cpu": lambda *a: ops.get_native_cpu().ttft_quantiles(*a),
    "torch": _torch,
    "kernel": _kernel,
    "kernel_by_row": _kernel_by_row,
}
IMPL_PARAMS = [pytest.param(k, marks=gpu) if k.startswith("kernel") else k for k in IMPLS]


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_oracle_table(impl):
    out = IMPLS[impl](*arrays(table()))
    assert out.shape == (len(table()), 2)
    worst = 0.0
    for (valid, q), c in zip(out, table()):
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], c["scv"])
        assert valid == 1.0, what
        if c["tol"] is None:  # no search ran: q is the prefill time
            assert abs(q / c["prefill"] - 1) <= FINAL_TOL, (what, q)
            continue
        t_got = (q - c["prefill"]) / ((1 + c["scv"]) / 2)
        worst = max(worst, abs(t_got / c["t"] - 1) / c["tol"])
        assert abs(t_got - c["t"]) <= c["t"] * c["tol"], (what, t_got, c["t"], c["tol"])
    print(f"{impl}: worst oracle error / bound = {worst:.3g}")


@pytest.mark.parametrize("impl", IMPL_PARAMS)
def test_rejected_inputs(impl):
    """Each rejected input between two valid rows: exactly (0, 0), and the
    valid rows bit-equal to their values when solved alone."""
    solve = IMPLS[impl]
    first, second = [c for c in table() if c["tol"] is not None and c["scv"] == 1.0
                     and int(c["row"][B.P_MAX_BATCH]) in (7, 64)][:2]
    top = float(oracle.rate_range(first["row"])[1] * 1000)
    bad = [dict(first, eps=e) for e in BAD_EPS + (0.0,)]
    bad += [dict(first, rate=r) for r in (NAN, INF, -INF, 0.0, -1.0, 1.01 * top)]
    bad += [dict(first, scv=-0.5), dict(first, row=_row(0))]
    cases = [c for b in bad for c in (first, b, second)]
    out = solve(*arrays(cases))
    alone = [solve(*arrays([c])) for c in (first, second)]
    assert alone[0][0, 0] == 1.0 and alone[1][0, 0] == 1.0
    assert not out[1::3].any()
    assert np.array_equal(out[0::3], np.tile(alone[0], (len(bad), 1)))
    assert np.array_equal(out[2::3], np.tile(alone[1], (len(bad), 1)))


@gpu
def test_routing_splits_by_batch_limit(monkeypatch):
    """N <= 700 rows interleaved with an N = 800 row: one launch with the
    small rows alone, the large one from the native CPU solver."""
    small = [c for c in table() if c["tol"] is not None][::7]
    row, lam, _ = _at(800, "0.99")
    big = {"row": row, "rate": float(lam * 1000), "eps": 0.05, "scv": 1.0}
    cases = [small[0], big, small[1], small[2], big]
    p, rates, eps, scv = arrays(cases)
    native, calls = ops.get_native(), []
    monkeypatch.setattr(native, "submit_quantile", lambda *a, _real=native.submit_quantile: (
        calls.append(len(a[0])), _real(*a))[1])
    out = ops.ttft_quantiles(p, rates, eps, device="cuda", scv=scv)
    assert calls == [3] and native.dispatch_pool_stats()[1] == 0
    assert np.array_equal(out[[0, 2, 3]], _kernel(*(v[[0, 2, 3]] for v in (p, rates, eps, scv))))
    assert np.array_equal(out[[1, 4]], IMPLS["cpu"](*(v[[1, 4]] for v in (p, rates, eps, scv))))
    assert (out[:, B.Q_VALID] == 1.0).all() and (out[[1, 4], B.Q_TTFT] > 0).all()


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=gpu)])
def test_fleet_percentile_prediction(device, monkeypatch):
    """test_fleet_percentile_knob's servers: under WVA_TTFT_PERCENTILE=95 every
    allocation carries the predicted p95 TTFT, equal to System.calculate()'s;
    with the knob unset nothing runs.  1e-4 guards the wiring (a wrong row,
    rate or eps is off by order 1); precision is the oracle test's job."""
    servers = [server_spec(f"s{i}:default", arrival_rate=rate, in_tokens=256, out_tokens=128,
                           max_batch=n) for i, (rate, n) in enumerate(
                               ((2400.0, 8), (9000.0, 16), (30000.0, 64)))]
    submits = []
    if device == "cuda":
        native = ops.get_native()
        monkeypatch.setattr(native, "submit_quantile", lambda *a, _real=native.submit_quantile: (
            submits.append(len(a[0])), _real(*a))[1])

    def sized(solver):
        system, _ = make_system(servers=servers)
        solver(system)
        return {(s.name, a): v for s in system.servers.values()
                for a, v in s.all_allocations.items()}

    unset = sized(BatchedAllocationSolver(device=device).calculate)
    assert unset and all(v.ttft_percentile == 0.0 for v in unset.values()) and not submits
    monkeypatch.setenv("WVA_TTFT_PERCENTILE", "95")
    want = sized(lambda s: s.calculate())
    got = sized(BatchedAllocationSolver(device=device).calculate)
    assert want and set(got) == set(want)
    for key, alloc in got.items():
        assert alloc.ttft_percentile == pytest.approx(want[key].ttft_percentile, rel=1e-4), key
        assert alloc.clone().ttft_percentile == alloc.ttft_percentile
    assert any(v.ttft_percentile > v.ttft for v in got.values())
    assert submits == ([len(got)] if device == "cuda" else [])
