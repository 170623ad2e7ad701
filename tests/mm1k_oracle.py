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
the code.

Helper module (like fixtures.py), not a conftest.
"""

from __future__ import annotations

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
