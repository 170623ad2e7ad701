"""Exact oracle for the waiting-time tail of the sizing model.

``exceedance(row, lam, t)`` is P(W > t) of an accepted arrival, by the direct
definition in 50-digit decimal arithmetic: the state probabilities from
``p[n+1] = p[n] * lam / mu``, and for each state n >= N the Erlang survival
``sum_{i<j} e^-x x^i / i!`` with j = n - N + 1 and x = mu_N * t.  No swapped
sum, no log space, no window: nothing of wva_amd's tail code.

``ttft_exceedance`` adds the contract's t(lam) (csrc/queue_core.h, "TTFT
percentile") from mm1k_oracle's evaluation.  Helper module, not a conftest.
"""

from decimal import Context, Decimal

import mm1k_oracle as oracle

_CTX = Context(prec=50)


def exceedance(row, lam, t) -> Decimal:
    """P(W > t) at arrival rate ``lam`` (req/ms), ``t`` in ms; 1 for t <= 0."""
    m = oracle.model_of(row)
    lam, t = Decimal(lam), Decimal(t)
    if t <= 0:
        return Decimal(1)
    add, mul, div = _CTX.add, _CTX.multiply, _CTX.divide
    p = Decimal(1)  # p[n], unnormalised
    accepted = Decimal(0)  # sum of p[0..K-1]: the states an accepted arrival sees
    x = mul(m.mu[-1], t)
    term = _CTX.exp(-x)  # e^-x x^i / i!, i = j - 1
    survival = Decimal(0)  # sum_{i<j}
    waiting = Decimal(0)  # sum_{n>=N} p[n] * survival(n - N + 1)
    for n in range(m.k):
        accepted = add(accepted, p)
        if n >= m.n:
            j = n - m.n + 1
            survival = add(survival, term)
            waiting = add(waiting, mul(p, survival))
            term = div(mul(term, x), Decimal(j))
        p = mul(p, div(lam, m.mu[min(n + 1, m.n) - 1]))
    return div(waiting, accepted)


def ttft_exceedance(row, lam, target_ttft, wait_scale=1) -> Decimal:
    """P(TTFT > target_ttft) at ``lam``: the wait, stretched by
    ``wait_scale``, against what prefill at the effective concurrency leaves."""
    at = oracle.evaluate(row, lam)
    prefill = at.ttft - at.wait
    return exceedance(row, lam, (Decimal(target_ttft) - prefill) / Decimal(wait_scale))
