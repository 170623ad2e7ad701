"""The percentile kernels against the exact oracles across the claimed
parameter range.

The six percentile modules (test_ops_ttft_tail, ..._ttft_tail_large_n,
..._ttft_quantile, ..._ttft_quantile_large_n, ..._itl_tail, ..._itl_quantile)
cover the N axis at one benign parameter point.  This module covers the other
axis, as test_ops_oracle_wide does for the mean sizing: rows drawn by that
module's ``draw`` (alpha 0.01 ... 1000 ms, beta 1e-4 ... 10, up to 32k input
and 8k output tokens) with a seed of its own, targets overwritten per family, N
mostly in 1..64 and otherwise on the edges ``EDGE_LIMITS`` (7680 on two rows
only: oracle time), and a per-row cs^2 from {0.25, 1, 4}.  Every known answer
comes from the decimal oracles through the six modules' own row-generic
builders, and every implementation in their ``IMPLS`` tables runs it: the
overlay kernels on the rows with N <= 700, everything else on all of them.

Bounds
------
Searched cases keep their module's bound: exact feasibility and replicas and
``rate_star`` within ``2e-6 * cond + 1e-9`` (TTFT tail), ``y_ref(rate_star)``
within 2e-6 eps (ITL tail), ``alpha + beta * b*`` within 2 ulp (ITL quantile).
The TTFT quantile is compared as q itself, ``|q - (ws t + prefill)| <= ws t
(2e-6 cond + 1e-9) + 2 ulp(q)``: at large alpha the prefill is 1e6 times t,
and subtracting it again would charge the implementations for a cancellation
they do not perform.  Where no search runs (a cap, an infeasible row, nobody
waits that often) a value holds ``FINAL_TOL + C_SCALE * 2^-53 * A`` with A =
``mm1k_oracle.log_table_scale``, as in test_ops_oracle_wide and derived the
same way: C_SCALE is 10x the worst scaled error of the Python definitions on
this very table, rounded up to a power of ten.  The kernels never set a bound.

Drops are decided from oracle quantities only (the wait floor, cond > 100, a
tie, a y outside (1e-280, 1), the ITL-tail builder's own placement rules),
counted by reason and printed; at most a quarter of a family's drawn cells may
go, and every edge N survives in every family.

The row contract: every ``INVALID_EDITS`` row of test_ops_row_contract goes
through the six entry points between valid rows of this table.
"""

import math
import time
import warnings
from collections import Counter
from decimal import Decimal as D
from functools import lru_cache

import numpy as np
import pytest

import mm1k_oracle as oracle
import test_ops_itl_quantile as IQ
import test_ops_itl_tail as I
import test_ops_ttft_quantile as Q
import test_ops_ttft_quantile_large_n as QL
import test_ops_ttft_tail as T
import test_ops_ttft_tail_large_n as TL
import ttft_tail_oracle as tail_oracle
from test_ops_oracle import FINAL_TOL, oracle_errors
from test_ops_oracle_wide import draw
from test_ops_row_contract import BASE_ROW, INVALID_EDITS
from wva_amd import ops
from wva_amd.ops import batched as B

SEED = 20250911
N_ROWS = 80
EDGE_LIMITS = (65, 255, 256, 257, 700, 701, 1024, 7680)
ROWS_PER_EDGE = {**{n: 3 for n in EDGE_LIMITS}, 7680: 2}
GPU_MAX_N = B.GPU_MAX_BATCH_LIMIT  # the overlay kernels' limit, 700
MAX_DROP_SHARE = 0.25
MIN_SEARCHED, MIN_NO_SEARCH = 15, 5
NO_SEARCH_STRIDE = 3  # every third row also gives its cases without a search

# worst err / (2^-53 * A) of the Python definitions where no search runs (CPU)
WORST_ANALYZER_RATIO = 0.427
C_SCALE = 1e1  # 10 x WORST_ANALYZER_RATIO, rounded up to a power of ten

FAMILIES = ("ttft_tail", "ttft_quantile", "itl_tail", "itl_quantile")
gpu = pytest.mark.gpu


def row_bound(scale):
    return FINAL_TOL + C_SCALE * 2.0**-53 * scale


def wide_rows():
    """(rows with no target set, their cs^2, the generator for the cells)."""
    rows = draw(N_ROWS, SEED)
    rng = np.random.default_rng(SEED + 1)
    edges = [n for n, k in ROWS_PER_EDGE.items() for _ in range(k)]
    rows[:, B.P_MAX_BATCH] = rng.integers(1, 65, N_ROWS)
    rows[rng.choice(N_ROWS, len(edges), replace=False), B.P_MAX_BATCH] = edges
    rows[:, B.P_TARGET_TTFT:B.P_TARGET_TPS + 1] = 0.0
    rows[:, B.P_TOTAL_RATE], rows[:, B.P_MIN_REPLICAS] = 10.0, 1.0
    return rows, rng.choice((0.25, 1.0, 4.0), N_ROWS), rng


def _fractions(n):
    """Where the waiting tail is worth a search: nearer saturation as N grows
    (at N = 7680 the wait at 0.99 of the range is 1e-12 of the service time)."""
    return ("0.5", "0.9", "0.99") if n <= 4 else ("0.9", "0.99", "0.999") if n <= 64 else (
        "0.99", "0.999") if n <= 700 else ("0.999", "0.9999")


def _scale(row, *lams):
    return max(oracle.log_table_scale(row, lam) for lam in lams)


def _ttft_tail_case(c):
    """A test_ops_ttft_tail case in the form test_ops_oracle.oracle_errors reads."""
    n = int(c["row"][B.P_MAX_BATCH])
    if c["lam"] is None:
        return dict(c, kind="below", N=n, feasible=False)
    ws, fin = (1 + D(c["scv"])) / 2, c["final"]
    scale = _scale(c["row"], c["lam"], fin.lam)
    case = dict(c, kind="ttft", N=n, feasible=True, replicas=4, scale=scale,
                final=fin._replace(ttft=ws * fin.wait + fin.ttft - fin.wait),
                final_tol=row_bound(scale))
    if c["rate_tol"] == T.FINAL_TOL:  # lam is the cap: known exactly
        case.update(kind="above", rate_tol=case["final_tol"])
    return case


def _ttft_tail_cell(row, f, mult, scv):
    """test_ops_ttft_tail.known_of, and one more drop rule.  cond is a central
    difference over lam (1 +- 1e-4).  The target moves with lam through the
    prefill time at the effective concurrency, and on these rows the prefill can
    be 1e4 waits: t = (target - prefill(lam)) / ws then falls to 0 inside the
    step, y jumps to 1, and the difference is no derivative (the benign table
    drops such cells by its wait floor, which is relative to the service time
    and does not see a prefill that large).  So the same quotient is formed
    again with a step of 1e-6, and a cell where the two differ by more than a
    half is dropped: its cond, and so its bound, is not known."""
    case, reason = T.known_of(row, f, mult, scv)
    if case is None:
        return None, reason
    h, lam, ws = D("1e-6"), case["lam"], (1 + D(scv)) / 2
    y_up, y_dn = (tail_oracle.ttft_exceedance(row, lam * s, row[B.P_TARGET_TTFT], ws)
                  for s in (1 + h, 1 - h))
    thr_up, thr_dn = (oracle.evaluate(row, lam * s).throughput for s in (1 + h, 1 - h))
    slope_y = abs(y_up - y_dn) / D(case["eps"])
    cond = (case["rate_tol"] - 1e-9) / 2e-6
    fine = float(abs(thr_up - thr_dn) * 1000 / case["rate_star"] / slope_y) if slope_y else math.inf
    if not abs(fine - cond) <= 0.5 * max(fine, cond):
        return None, "difference_is_no_derivative"
    return _ttft_tail_case(case), None


def _itl_tail_cells(row, scv, u):
    """(searched case or None, drop reason): c = the drawn share u of 1..N-1,
    the target between decode_time(c) and decode_time(c + 1), eps the share u of
    the way (in logs) through the range test_ops_itl_tail._case allows."""
    n = int(row[B.P_MAX_BATCH])
    c = 1 + int(u * (n - 1))
    row[B.P_TARGET_ITL] = row[B.P_ALPHA] + row[B.P_BETA] * c + row[B.P_BETA] / 2
    y0, y1 = I.eps_range(row)
    low, high = max(10 * y0, 1e-9), y1 / 10
    if not low * 1.01 < high:
        return None, "eps_near_range_end"
    eps = float(np.exp(np.log(low * 1.01) + u * (np.log(high) - np.log(low * 1.01))))
    lam, reason = I.binding_lam(row, eps)
    if reason:
        return None, reason
    case = I._case(row, c, eps, scv=scv)
    at = oracle.evaluate(row, lam)
    if scv == 4.0 and at.ttft > 0:  # the TTFT tail too, where it is clearly the looser one
        row[B.P_TARGET_TTFT] = 10 * float(at.ttft)
        beyond = tail_oracle.ttft_exceedance(row, lam * 1.001, row[B.P_TARGET_TTFT], D("2.5"))
        if beyond < D("0.025"):
            case["ttft_eps"] = 0.05
        else:
            row[B.P_TARGET_TTFT] = 0.0
    return case, None


def _itl_no_search(row, scv):
    cases = []
    for c in (0, int(row[B.P_MAX_BATCH])):  # below decode_time(1); above decode_time(N)
        r = row.copy()
        r[B.P_TARGET_ITL] = r[B.P_ALPHA] + r[B.P_BETA] * c + r[B.P_BETA] / 2
        case = I._case(r, c, 0.05, scv=scv)
        if case["kind"] == "cap":
            case["scale"] = _scale(r, case["lam"])
            case["final_tol"] = row_bound(case["scale"])
        cases.append(case)
    return cases


def _keep(table, family, case, reason):
    table[family]["cells"] += 1
    if case is None:
        table[family]["drops"][reason] += 1
    else:
        table[family]["searched"].append(case)


@lru_cache(maxsize=None)
def wide_table():
    started = time.perf_counter()
    rows, scvs, rng = wide_rows()
    table = {f: {"searched": [], "no_search": [], "cells": 0, "drops": Counter()} for f in FAMILIES}
    for i, (row, scv) in enumerate(zip(rows, scvs)):
        n, scv = int(row[B.P_MAX_BATCH]), float(scv)
        for mult in ("0.5", "3"):
            f = str(rng.choice(_fractions(n)))
            _keep(table, "ttft_tail", *_ttft_tail_cell(row.copy(), f, mult, scv))
            _keep(table, "ttft_quantile", *Q.known_of(row.copy(), f, mult, scv))
        if n >= 2:
            _keep(table, "itl_tail", *_itl_tail_cells(row.copy(), scv, rng.random()))
        # the ITL quantile: steered to an answer inside 2..N-1 by a high load and a large eps
        for low, high, eps in ((0.9, 1.0, 0.5), (0.8, 1.0, 0.05), (0.3, 0.95, 0.001)):
            case = IQ.case_of(row.copy(), float(rng.uniform(low, high)), eps)
            _keep(table, "itl_quantile", None if case["tie"] else case, "tie")
        if i % NO_SEARCH_STRIDE == 0:
            table["ttft_tail"]["no_search"] += [_ttft_tail_case(c) for c in T.no_search_of(row.copy())]
            case = Q.nobody_waits_of(row.copy(), "0.5", scv)
            at = oracle.evaluate(row, D(case["rate"]) / 1000)
            case["scale"] = _scale(row, at.lam)
            case["spread"] = float(at.ttft - at.wait + at.serv)  # what oracle_errors scales a TTFT by
            table["ttft_quantile"]["no_search"].append(case)
            table["itl_tail"]["no_search"] += _itl_no_search(row, scv)
    # the ITL quantile searches nothing where the answer is the batch limit itself
    found = table["itl_quantile"]
    found["no_search"] = [c for c in found["searched"] if c["b"] == c["row"][B.P_MAX_BATCH]]
    found["searched"] = [c for c in found["searched"] if c["b"] < c["row"][B.P_MAX_BATCH]]
    print(f"wide percentile table built in {time.perf_counter() - started:.1f} s")
    for name, t in table.items():
        dropped = sum(t["drops"].values())
        print(f"  {name}: {len(t['searched'])} searched, {len(t['no_search'])} without a search; "
              f"dropped {dropped} of {t['cells']} cells: {dict(t['drops'])}")
    for name, t in table.items():
        dropped = sum(t["drops"].values())
        assert dropped <= MAX_DROP_SHARE * t["cells"], (name, dropped, t["cells"])
        assert len(t["searched"]) >= MIN_SEARCHED and len(t["no_search"]) >= MIN_NO_SEARCH, name
        kept = {int(c["row"][B.P_MAX_BATCH]) for c in t["searched"] + t["no_search"]}
        assert kept >= set(EDGE_LIMITS), (name, set(EDGE_LIMITS) - kept)
    many = [c for c in found["searched"] + found["no_search"] if c["row"][B.P_MAX_BATCH] >= 2]
    inside = sum(1 < c["b"] < c["row"][B.P_MAX_BATCH] for c in many)
    print(f"  itl_quantile: 1 < b* < N in {inside} of {len(many)} cases with N >= 2")
    assert 3 * inside >= len(many)
    assert any(c["ttft_eps"] and c["scv"] == 4.0 for c in table["itl_tail"]["searched"])
    return table


def cases_of(family, max_n):
    t = wide_table()[family]
    return [c for c in t["searched"] + t["no_search"] if c["row"][B.P_MAX_BATCH] <= max_n]


# ---------------------------------------------------------------------------
# The checks: each returns (worst searched error / its bound, worst scaled error
# where no search ran) and raises on the first case that misses its bound.
# ---------------------------------------------------------------------------

def check_ttft_tail(out, cases, _solve):
    worst, problems = oracle_errors(out, cases)
    assert not problems, f"{len(problems)} mismatches, first: " + "; ".join(problems[:5])
    return worst["rate_vs_bound"], worst.get("scaled", 0.0)


def check_ttft_quantile(out, cases, _solve):
    assert out.shape == (len(cases), 2)
    searched = scaled = 0.0
    for (valid, q), c in zip(out, cases):
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], c["scv"], q)
        assert valid == 1.0, what
        if c["tol"] is None:  # no search ran: q is the prefill time
            err = abs(q - c["prefill"]) / c["spread"]
            scaled = max(scaled, err / (2.0**-53 * c["scale"]))
            assert err <= row_bound(c["scale"]), (what, c["prefill"], err)
            continue
        wait = (1 + c["scv"]) / 2 * c["t"]
        want = wait + c["prefill"]
        bound = wait * c["tol"] + 2 * np.spacing(want)
        searched = max(searched, abs(q - want) / bound)
        assert abs(q - want) <= bound, (what, want, abs(q - want) / bound)
    return searched, scaled


def check_itl_tail(out, cases, solve):
    I.check(out, cases, solve)  # raises; the figures below are for the record
    searched = scaled = 0.0
    for res, c in zip(out, cases):
        if c["kind"] == "itl":
            y = float(I.y_ref(c["row"], res[B.R_RATE_STAR] / 1000, c["row"][B.P_TARGET_ITL]))
            searched = max(searched, abs(y / c["eps"] - 1) / 2e-6)
        elif c["kind"] == "cap":
            want = float(oracle.evaluate(c["row"], c["lam"]).throughput) * 1000
            scaled = max(scaled, abs(res[B.R_RATE_STAR] / want - 1) / (2.0**-53 * c["scale"]))
    return searched, scaled


def check_itl_quantile(out, cases, _solve):
    assert out.shape == (len(cases), 2)
    worst = 0.0
    for (valid, q), c in zip(out, cases):
        want = c["row"][B.P_ALPHA] + c["row"][B.P_BETA] * c["b"]
        what = (int(c["row"][B.P_MAX_BATCH]), c["rate"], c["eps"], c["b"], q, want)
        worst = max(worst, abs(q - want) / (2 * np.spacing(want)))
        assert valid == 1.0 and abs(q - want) <= 2 * np.spacing(want), what
    return worst, 0.0


CHECKS = {"ttft_tail": check_ttft_tail, "ttft_quantile": check_ttft_quantile,
          "itl_tail": check_itl_tail, "itl_quantile": check_itl_quantile}
ARRAYS = {"ttft_tail": T.arrays, "ttft_quantile": Q.arrays, "itl_tail": I.arrays,
          "itl_quantile": IQ.arrays}
ALL_N = B.GPU_COMPACT_MAX_BATCH_LIMIT


def _implementations():
    """(family, name) -> (solver, largest N it takes): every entry of the six
    modules' IMPLS.  The overlay kernels stop at N = 700."""
    impls = {}
    for name, solve in T.IMPLS.items():
        impls["ttft_tail", name] = (solve, GPU_MAX_N if name.startswith("kernel") else ALL_N)
    for name, (solve, cases) in TL.IMPLS.items():
        if cases is TL.table:  # the *_small_n entries are the same solvers
            impls["ttft_tail", name.replace("kernel", "kernel_compact")] = (solve, ALL_N)
    for name, solve in Q.IMPLS.items():
        impls["ttft_quantile", name] = (solve, GPU_MAX_N if name.startswith("kernel") else ALL_N)
    for name, solve in QL.IMPLS.items():
        impls["ttft_quantile", name.replace("kernel", "kernel_compact")] = (solve, ALL_N)
    for name, solve in I.IMPLS.items():
        impls["itl_tail", name] = (solve, ALL_N)
    for name, solve in IQ.IMPLS.items():
        impls["itl_quantile", name] = (solve, ALL_N)
    return impls


IMPLS = _implementations()
KERNELS = [k for k in IMPLS if k[1].startswith("kernel")]
IMPL_PARAMS = [pytest.param(*k, marks=gpu if k in KERNELS else (), id="-".join(k)) for k in IMPLS]


def test_table_spans_the_claimed_ranges():
    rows = wide_rows()[0]
    assert rows[:, B.P_ALPHA].min() < 0.1 and rows[:, B.P_ALPHA].max() > 100
    assert rows[:, B.P_BETA].min() < 1e-3 and rows[:, B.P_BETA].max() > 1
    assert rows[:, B.P_IN_TOKENS].max() > 16384 and (rows[:, B.P_IN_TOKENS] == 0).any()
    assert rows[:, B.P_OUT_TOKENS].max() > 4096 and (rows[:, B.P_OUT_TOKENS] == 1).any()
    assert (rows[:, B.P_MAX_BATCH] <= 64).sum() * 2 > N_ROWS
    assert (rows[:, B.P_MAX_BATCH] == 7680).sum() <= 3
    for family in FAMILIES:  # the rows mix every cs^2 where the family takes one
        assert {c.get("scv", 1.0) for c in cases_of(family, ALL_N)} >= (
            {1.0} if family == "itl_quantile" else {0.25, 1.0, 4.0})


def test_c_scale_comes_from_the_analyzer():
    """C_SCALE is derived, not chosen: 10x the worst scaled error of the Python
    definitions where no search runs, rounded up to a power of ten."""
    assert C_SCALE == 10.0 ** math.ceil(math.log10(10.0 * WORST_ANALYZER_RATIO))
    worst = 0.0
    for family in FAMILIES[:3]:
        cases = cases_of(family, ALL_N)
        solve = IMPLS[family, "python"][0]
        worst = max(worst, CHECKS[family](solve(*ARRAYS[family](cases)), cases, solve)[1])
    print(f"Python definitions, worst err / (2^-53 A): {worst:.3g}")
    assert worst <= C_SCALE / 10.0


@pytest.mark.parametrize("family,impl", IMPL_PARAMS)
def test_wide_table(family, impl):
    solve, max_n = IMPLS[family, impl]
    cases = cases_of(family, max_n)
    assert len(cases) <= 250
    searched, scaled = CHECKS[family](solve(*ARRAYS[family](cases)), cases, solve)
    print(f"{family} {impl}: {len(cases)} cases, worst searched error / bound = {searched:.3g}, "
          f"worst err / (2^-53 A) where no search runs = {scaled:.3g}")


@gpu
@pytest.mark.parametrize("family,impl", [k for k in KERNELS if not k[1].endswith("by_row")],
                         ids="-".join)
def test_kernel_rows_alone(family, impl):
    """Every seventh row in a launch of its own: bit-equal to its row of the
    batch, which mixes J from 10 to 76800 in one launch."""
    solve, max_n = IMPLS[family, impl]
    args = ARRAYS[family](cases_of(family, max_n))
    batch = solve(*args)
    for i in range(0, len(batch), 7):
        assert np.array_equal(solve(*(v[i:i + 1] for v in args)), batch[i:i + 1]), i


# ---------------------------------------------------------------------------
# Row contract: INVALID_EDITS through the six entry points
# ---------------------------------------------------------------------------

def _invalid(family):
    """The family's arguments for BASE_ROW, with both targets set, under every
    invalid edit: eps = 0.05 and, for the quantiles, a valid rate."""
    base = np.array(BASE_ROW)
    base[B.P_TARGET_TTFT], base[B.P_TARGET_ITL] = 500.0, 6.0
    rows = np.tile(base, (len(INVALID_EDITS), 1))
    for row, (field, value) in zip(rows, INVALID_EDITS):
        row[field] = value
    k = len(rows)
    ones, eps = np.ones(k), np.full(k, 0.05)
    rates = np.full(k, 0.5 * float(oracle.rate_range(base)[1]) * 1000)
    return {"ttft_tail": (rows, ones, eps), "ttft_quantile": (rows, rates, eps, ones),
            "itl_tail": (rows, ones, np.zeros(k), eps), "itl_quantile": (rows, rates, eps)}[family]


def _limit(p, most):
    return min(int(B._valid_batch_limits(p).max()), most)


def _contract_kernels():
    """The seven launches with the LDS sized from the valid rows alone (the
    modules' own wrappers take max(N) of every row, NaN and 1e300 included)."""
    native = ops.get_native()
    return {
        ("ttft_tail", "kernel"): lambda p, scv, eps: native.collect(
            native.submit_tail(p, _limit(p, GPU_MAX_N), eps, scv)),
        ("ttft_tail", "kernel_compact"): lambda p, scv, eps: native.collect(
            native.submit_tail_compact(p, _limit(p, ALL_N), eps, scv)),
        ("ttft_quantile", "kernel"): Q._kernel,
        ("ttft_quantile", "kernel_compact"): QL._kernel,
        ("itl_tail", "kernel"): lambda p, scv, tt, itl: native.collect(
            native.submit_ptile(p, _limit(p, ALL_N), itl, tt, scv, False)),
        ("itl_tail", "kernel_split"): lambda p, scv, tt, itl: native.collect(
            native.submit_ptile(p, _limit(p, ALL_N), itl, tt, scv, True)),
        ("itl_quantile", "kernel"): IQ._kernel,
    }


CONTRACT_PARAMS = [pytest.param(*k, marks=gpu if k in KERNELS else (), id="-".join(k))
                   for k in IMPLS if not k[1].endswith("by_row")]


@pytest.mark.parametrize("family,impl", CONTRACT_PARAMS)
def test_invalid_rows_are_zero_rows(family, impl):
    """Two invalid rows after every valid one: the invalid ones come back
    all-zero, the valid ones bit-equal to their values without them."""
    is_kernel = (family, impl) in KERNELS
    solve = _contract_kernels()[family, impl] if is_kernel else IMPLS[family, impl][0]
    bad = _invalid(family)
    n = len(bad[0]) // 2
    assert 2 * n == len(INVALID_EDITS)
    searched = [c for c in wide_table()[family]["searched"] if c["row"][B.P_MAX_BATCH] <= GPU_MAX_N]
    valid = tuple(v[:n] for v in ARRAYS[family](searched))
    assert len(valid[0]) == n
    mixed = []
    for v, b in zip(valid, bad):
        both = np.empty((3 * n,) + v.shape[1:])
        both[0::3], both[1::3], both[2::3] = v, b[0::2], b[1::2]
        mixed.append(both)
    if is_kernel:
        out, alone = solve(*mixed), solve(*valid)
    else:
        with warnings.catch_warnings(), np.errstate(divide="raise", invalid="raise"):
            warnings.simplefilter("error")
            out, alone = solve(*mixed), solve(*valid)
    assert alone[:, 0].all(), "a valid row came back rejected"
    assert not out[1::3].any() and not out[2::3].any()
    assert np.array_equal(out[0::3], alone)
