"""The exact oracle with the M/G/1 wait scaling (per-row service-time cs^2).

``mm1k_oracle.oracle_solve`` is reused unchanged: it forms every quantity it
decides on from ``mm1k_oracle.evaluate``, so swapping that one function for a
wrapper that scales the wait solves the corrected problem with the very same
drop rules, margins and bisection.  The wrapper applies the *definition* of
the correction (csrc/queue_core.h header, ops/batched.py docstring):

    wait_scale = (1 + scv) / 2
    wait' = wait * wait_scale            (the wait >= 0 clamp comes first)
    ttft' = wait' + prefill(eff_conc)    (prefill = ttft - wait of the oracle)

in 50-digit decimal arithmetic; throughput, ITL, rho and everything else are
untouched.  It shares no code with the solvers.

Helper module (like mm1k_oracle.py and fixtures.py), not a conftest.
"""

from __future__ import annotations

import contextlib
from decimal import Decimal

import mm1k_oracle as oracle

_CTX = oracle._CTX


def wait_scale(scv) -> Decimal:
    return _CTX.divide(_CTX.add(Decimal(1), Decimal(float(scv))), Decimal(2))


@contextlib.contextmanager
def scaled_evaluate(scv):
    """While active, ``mm1k_oracle.evaluate`` returns the cs^2-corrected
    evaluation; the real one is restored on exit, whatever happens."""
    s = wait_scale(scv)
    real = oracle.evaluate

    def evaluate(row, lam):
        e = real(row, lam)
        wait = _CTX.multiply(e.wait, s)
        return e._replace(wait=wait, ttft=_CTX.add(wait, _CTX.subtract(e.ttft, e.wait)))

    oracle.evaluate = evaluate
    try:
        yield
    finally:
        oracle.evaluate = real


def evaluate(row, lam, scv):
    """Corrected oracle evaluation of ``row`` at ``lam`` (req/ms)."""
    with scaled_evaluate(scv):
        return oracle.evaluate(row, lam)


def oracle_solve(row, scv):
    """``mm1k_oracle.oracle_solve`` of ``row`` under service-time cs^2
    ``scv``: ``(case, None)`` or ``(None, reason)``; a kept case also carries
    its ``scv``."""
    with scaled_evaluate(scv):
        case, reason = oracle.oracle_solve(row)
    if case is not None:
        case["scv"] = float(scv)
    return case, reason
