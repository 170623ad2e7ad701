"""Exact oracle for the state-dependent M/M/1/K sizing model.

Evaluates one problem row at one arrival rate by the direct birth-death
recursion in 50-digit decimal arithmetic:

    p[0] = 1,  p[n+1] = p[n] * lam / mu(min(n+1, N)),  n < K = 11 * N

normalised by the full sum.  It deliberately shares nothing with wva_amd:
no log space, no geometric tail, no windowing, no numpy — only + - * / on
``decimal.Decimal``, whose exponent range makes the unnormalised products
(1e+-20000 and beyond) harmless.  Inputs are converted with
``Decimal(float)``, which is exact, so the oracle answers the very problem
the float64 solvers were given.

Derived quantities follow the definitions of csrc/queue_core.h (Stats,
effective_concurrency, eval_ttft_of, eval_itl_of) — the *definitions*, not
the code.  ``oracle_solve`` goes one step further and solves a whole sizing
row (targets, TPS cap, replicas) from these evaluations, again following the
definitions of queue_host.h's solve_one and never its code.

Helper module (like fixtures.py), not a conftest.
"""

from __future__ import annotations

import math
from decimal import Context, Decimal
from functools import lru_cache
from typing import NamedTuple

# problem-row columns (csrc/queue_core.h ProblemField)
ALPHA, BETA, GAMMA, DELTA, IN_TOKENS, OUT_TOKENS, MAX_BATCH = range(7)

QUEUE_TO_BATCH_RATIO = 10
EPSILON = Decimal("0.001")

_CTX = Context(prec=50)


class Exact(NamedTuple):
    """Oracle evaluation at one arrival rate; every field a Decimal."""

    lam: Decimal  # req/ms
    throughput: Decimal  # req/ms
    n_sys: Decimal
    n_serv: Decimal
    serv: Decimal  # ms
    wait: Decimal  # ms
    eff_conc: Decimal
    itl: Decimal  # ms
    ttft: Decimal  # ms
    rho: Decimal


class Model(NamedTuple):
    alpha: Decimal
    beta: Decimal
    gamma: Decimal
    delta: Decimal
    in_tokens: Decimal
    out_tokens: int
    n: int  # batch limit N
    k: int  # occupancy bound K
    mu: tuple  # mu[b-1] = service rate at batch b, b in [1, N] (req/ms)
    lam_min: Decimal
    lam_max: Decimal


def _prefill(m: Model, batch: Decimal) -> Decimal:
    if m.in_tokens == 0:
        return Decimal(0)
    return _CTX.add(m.gamma, _CTX.multiply(_CTX.multiply(m.delta, m.in_tokens), batch))


def _decode(m: Model, batch: Decimal) -> Decimal:
    return _CTX.add(m.alpha, _CTX.multiply(m.beta, batch))


@lru_cache(maxsize=None)
def _model(alpha, beta, gamma, delta, in_tokens, out_tokens, max_batch) -> Model:
    n = int(max_batch)
    out = int(out_tokens)
    num_decode = out - 1
    if in_tokens == 0 and out == 1:
        num_decode = 1
    m = Model(
        Decimal(alpha), Decimal(beta), Decimal(gamma), Decimal(delta),
        Decimal(in_tokens), out, n, n * (1 + QUEUE_TO_BATCH_RATIO), (), Decimal(0), Decimal(0),
    )
    mu = []
    for b in range(1, n + 1):
        bd = Decimal(b)
        t = _CTX.add(_prefill(m, bd), _CTX.multiply(Decimal(num_decode), _decode(m, bd)))
        mu.append(_CTX.divide(bd, t))
    lam_min = _CTX.multiply(mu[0], EPSILON)
    lam_max = _CTX.multiply(mu[-1], _CTX.subtract(Decimal(1), EPSILON))
    return m._replace(mu=tuple(mu), lam_min=lam_min, lam_max=lam_max)


def model_of(row) -> Model:
    """Model constants (and the stable rate range) of a problem row."""
    return _model(*(float(row[c]) for c in range(MAX_BATCH + 1)))


def rate_range(row):
    """(lam_min, lam_max) in req/ms: mu(1)*1e-3 and mu(N)*(1 - 1e-3)."""
    m = model_of(row)
    return m.lam_min, m.lam_max


def evaluate(row, lam) -> Exact:
    """Exact model evaluation of problem ``row`` at ``lam`` (req/ms).

    ``lam`` may be a float (converted exactly) or a Decimal.
    """
    m = model_of(row)
    lam = Decimal(lam)
    add, mul, div, sub = _CTX.add, _CTX.multiply, _CTX.divide, _CTX.subtract
    n_batch, k = m.n, m.k

    # lam / mu(b), b in [1, N]: one division per distinct service rate
    ratio = [div(lam, mu_b) for mu_b in m.mu]
    p = Decimal(1)
    total = Decimal(1)  # sum p[n]
    first = Decimal(0)  # sum n p[n]
    total_n = first_n = None  # the same sums over n <= N
    for n in range(k):
        p = mul(p, ratio[min(n + 1, n_batch) - 1])  # p[n+1]
        total = add(total, p)
        first = add(first, mul(Decimal(n + 1), p))
        if n + 1 == n_batch:
            total_n, first_n = total, first
    p_k = div(p, total)

    throughput = mul(lam, sub(Decimal(1), p_k))
    n_sys = div(first, total)
    n_serv = add(
        div(first_n, total), mul(sub(Decimal(1), div(total_n, total)), Decimal(n_batch))
    )
    if throughput == 0:
        serv = wait = Decimal(0)
    else:
        serv = div(n_serv, throughput)
        wait = max(sub(div(n_sys, throughput), serv), Decimal(0))

    # effective concurrency: solve prefill(n) + (out-1)*decode(n) = serv
    tokens = Decimal(m.out_tokens - 1)
    numer = sub(serv, add(m.gamma, mul(m.alpha, tokens)))
    denom = add(mul(m.delta, m.in_tokens), mul(m.beta, tokens))
    if denom == 0:
        eff = Decimal(n_batch) if numer > 0 else Decimal(0)
    else:
        eff = min(max(div(numer, denom), Decimal(0)), Decimal(n_batch))

    rho = min(max(div(n_serv, Decimal(n_batch)), Decimal(0)), Decimal(1))
    return Exact(
        lam=lam, throughput=throughput, n_sys=n_sys, n_serv=n_serv, serv=serv,
        wait=wait, eff_conc=eff, itl=_decode(m, eff), ttft=add(wait, _prefill(m, eff)),
        rho=rho,
    )


# ---------------------------------------------------------------------------
# Oracle-side solve of an arbitrary (valid) sizing row
# ---------------------------------------------------------------------------

TARGET_TTFT, TARGET_ITL, TARGET_TPS, TOTAL_RATE, MIN_REPLICAS = 7, 8, 9, 10, 11

STABILITY_FRACTION = Decimal("0.1")  # TPS cap: lam_max * (1 - 0.1)

# margins of the drop rules (all relative)
BOUNDARY_MARGIN = Decimal("1e-4")  # target vs y(lam_min), y(lam_max), y at a rival lam
FLAT_SPREAD = Decimal("1e-5")  # |y(lam_max) - y(lam_min)| below this: flat curve
MIN_SLOPE = Decimal("1e-3")  # |dln y / dln lam| of a binding target
MAX_COND = 100.0
WAIT_FLOOR = Decimal("1e-4")  # decode-only TTFT: wait >= floor * serv
# a solver's lam for a binding target is off by up to its 1e-6 stop in y
# over the slope, <= 1e-3 relative; rivals (the other target, the cap) must be this clear of it
RIVAL_MARGIN = Decimal("2e-3")
LAM_MAX_MARGIN = Decimal("1e-6")  # per-replica rate vs lam_max * 1000
BISECT_REL = Decimal("1e-10")  # bracket width at which the bisection stops
_H = Decimal("1e-4")  # central-difference step of the slopes
KNOWN_RATE_TOL = 1e-9  # replica-quotient margin where lam is a cap


def log_table_scale(row, lam) -> float:
    """A = max(|cum[K-1]|, K * |ln lam|): the magnitude of the two terms
    whose difference is the log-probability of the last state.  float64
    solvers that work in log space lose 2^-53 * A of absolute precision in
    it, which sets their achievable accuracy at this row and rate.  A scale,
    not an answer: plain float logs of the oracle's rates are enough."""
    m = model_of(row)
    cum = sum(math.log(float(mu_b)) for mu_b in m.mu) + (m.k - m.n) * math.log(float(m.mu[-1]))
    return max(abs(cum), m.k * abs(math.log(float(lam))))


def _bisect(row, name, target, lo, hi):
    """lam in [lo, hi] with y(lam) = target, y increasing, y(lo) < target <
    y(hi): plain halving (~34 steps plus log2(hi / lam*)) in Decimal."""
    two = Decimal(2)
    while hi - lo > lo * BISECT_REL:
        mid = (lo + hi) / two
        if getattr(evaluate(row, mid), name) < target:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / two


def oracle_solve(row):
    """Solve one valid sizing row with the oracle alone.

    Follows the definitions of csrc/queue_core.h / queue_host.h: per-target
    boundary classification (target below the curve -> infeasible, above ->
    lam_max), lam* of each active target, the TPS cap 0.9 * lam_max, lam =
    the smallest of them, rate_star = throughput(lam) * 1000, replicas =
    max(ceil(total / rate_star), trunc(min_replicas)), rejection of a
    per-replica rate above lam_max * 1000, and the final evaluation at total /
    replicas.

    Returns ``(case, None)`` or ``(None, reason)``.  ``case`` has the keys
    test_ops_oracle.oracle_errors consumes (kind, N, feasible, rate_tol,
    rate_star, replicas, final, row) plus ``bound`` (what fixed lam: "ttft",
    "itl", "tps" or "none"), ``has_above`` and ``scale`` (log_table_scale).
    A row is dropped, with a named reason, whenever a float64 solver that is
    correct to its own tolerances could legitimately decide differently;
    every such decision is made here, from oracle quantities only.
    """
    one = Decimal(1)
    m = model_of(row)
    n = m.n
    lam_min, lam_max = m.lam_min, m.lam_max
    targets = {
        "ttft": Decimal(float(row[TARGET_TTFT])),
        "itl": Decimal(float(row[TARGET_ITL])),
    }
    tps = float(row[TARGET_TPS])
    decode_only = m.in_tokens == 0
    bottom, top = evaluate(row, lam_min), evaluate(row, lam_max)

    def infeasible():
        return {"kind": "below", "N": n, "feasible": False, "rate_tol": None,
                "bound": None, "has_above": False, "row": row.copy()}, None

    within, has_above = [], False
    for name in ("ttft", "itl"):
        t = targets[name]
        if t <= 0:
            continue
        y0, y1 = getattr(bottom, name), getattr(top, name)
        if abs(t - y0) <= BOUNDARY_MARGIN * abs(y0) or abs(t - y1) <= BOUNDARY_MARGIN * abs(y1):
            return None, "target_on_range_end"
        if name == "ttft" and decode_only and t < y0 and bottom.wait < WAIT_FLOOR * bottom.serv:
            return None, "wait_under_cancellation_floor"
        if abs(y1 - y0) < FLAT_SPREAD * max(abs(y0), abs(y1)):
            # flat curve: the solvers classify by value alone; only a
            # target clear of the whole span is decided the same way
            if t > max(y0, y1) * (one + BOUNDARY_MARGIN):
                has_above = True
                continue
            if t < min(y0, y1) * (one - BOUNDARY_MARGIN):
                return infeasible()
            return None, "flat_curve"
        if y1 < y0:
            return None, "decreasing_curve"
        if t < y0:
            return infeasible()  # below the reachable region
        if t > y1:
            has_above = True  # lam* = lam_max
            continue
        within.append(name)

    # the winner so far: a cap is exact, a bisected lam is not
    cap = lam_max * (one - STABILITY_FRACTION) if tps > 0 else lam_max
    lam, bound = cap, ("tps" if tps > 0 else "none")
    for name in within:
        t = targets[name]
        if bound in ("tps", "none"):
            y_cap = getattr(top if bound == "none" else evaluate(row, cap), name)
            if y_cap < t * (one - BOUNDARY_MARGIN):
                continue  # this target's lam* lies above the cap
            if not y_cap > t * (one + BOUNDARY_MARGIN):
                return None, "target_ties_with_cap"
            lam_t = _bisect(row, name, t, lam_min, cap)
            if not lam_t * (one + RIVAL_MARGIN) < cap:
                return None, "target_ties_with_cap"
            lam, bound = lam_t, name
        else:
            # a bisected winner exists: is this target clearly looser?
            if getattr(evaluate(row, lam * (one + RIVAL_MARGIN)), name) < t * (one - BOUNDARY_MARGIN):
                continue
            lam_t = _bisect(row, name, t, lam_min, lam_max)
            rival = targets[bound]
            if not getattr(evaluate(row, lam_t * (one + RIVAL_MARGIN)), bound) < rival * (
                one - BOUNDARY_MARGIN
            ):
                return None, "targets_tie"
            lam, bound = lam_t, name

    at = evaluate(row, lam)
    if bound in ("ttft", "itl"):
        up, dn = evaluate(row, lam * (one + _H)), evaluate(row, lam * (one - _H))

        def slope(field):  # |dln y / dln lam|, central difference
            return abs((getattr(up, field) - getattr(dn, field)) / getattr(at, field) / (2 * _H))

        s = slope(bound)
        if s < MIN_SLOPE:
            return None, "binding_slope_too_small"
        cond = float(slope("throughput") / s)
        if cond > MAX_COND:
            return None, "ill_conditioned"
        if bound == "ttft" and decode_only and at.wait < WAIT_FLOOR * at.serv:
            return None, "wait_under_cancellation_floor"
        rate_tol = 2e-6 * cond + 1e-9
        quotient_tol = rate_tol
    else:
        rate_tol = None  # lam is known exactly: the caller's final tolerance
        quotient_tol = KNOWN_RATE_TOL

    rate_star = at.throughput * 1000  # req/s
    total = Decimal(float(row[TOTAL_RATE]))
    quotient = total / rate_star
    nearest = quotient.to_integral_value()
    # ceil() cannot flip at 0 for a positive quotient: integers >= 1 only
    if nearest >= 1 and abs(quotient - nearest) <= Decimal(10 * quotient_tol) * nearest:
        return None, "replica_quotient_on_integer"
    replicas = max(int(quotient.to_integral_value(rounding="ROUND_CEILING")),
                   int(float(row[MIN_REPLICAS])))
    if replicas <= 0:
        return infeasible()
    rate = total / replicas  # req/s per replica
    if not rate > 0:
        return infeasible()
    if abs(rate / (lam_max * 1000) - one) <= LAM_MAX_MARGIN:
        return None, "rate_on_lam_max"
    if rate > lam_max * 1000:
        return infeasible()
    final = evaluate(row, rate / 1000)
    kind = bound if bound in ("ttft", "itl") else ("above" if has_above else bound)
    return {
        "kind": kind, "N": n, "feasible": True, "rate_tol": rate_tol, "bound": bound,
        "has_above": has_above, "rate_star": rate_star, "replicas": replicas,
        "final": final, "row": row.copy(),
        "scale": max(log_table_scale(row, lam), log_table_scale(row, rate / 1000)),
    }, None
