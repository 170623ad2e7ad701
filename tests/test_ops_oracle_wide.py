"""Sizing solvers against the exact oracle across the claimed parameter range.

test_ops_oracle.py covers every lane, chunk and LDS edge in N at one benign
parameter point.  This module covers the other axis: rows drawn over the whole
range the project claims (alpha 0.01 ... 1000 ms, beta 1e-4 ... 10, up to 32k
input and 8k output tokens, any mix of targets), each *solved by the oracle*
(mm1k_oracle.oracle_solve: Decimal bisection for lam*, TPS cap, replicas,
final evaluation) and run through every implementation.  The GPU kernels and
the host C++ share csrc/queue_core.h, so comparing them with each other cannot
see a mistake in that shared math; the oracle shares nothing with either.

Rows on which a correct float64 solver may legitimately decide differently
(target on a range end, flat or ill-conditioned curve, replica quotient on an
integer, ...) are dropped when the table is built, from oracle quantities
only, with the reason counted and printed; at most MAX_DROP_SHARE may go.

Tolerances
----------
Feasibility and replicas are exact.  ``rate_star`` of a binding TTFT/ITL
target: ``2e-6 * cond + 1e-9`` as in test_ops_oracle.py.  Final ITL, TTFT,
rho, and ``rate_star`` where lam is a cap, are bounded per row by

    FINAL_TOL + C_SCALE * 2^-53 * A,   A = max(|cum[K-1]|, K * |ln lam|)

because every log-space float64 solver forms log p[n] = n ln lam - cum[n-1]
and so loses 2^-53 * A of absolute precision in it; away from the benign
point A reaches 1e5 and more, and 1e-11 is not attainable by any of them.
C_SCALE is 10x the worst ``err / (2^-53 * A)`` of the Python analyzer — the
semantic reference, whose arithmetic (numpy, full sweeps) differs from the
kernels' — on this very table, rounded up to a power of ten; the 10x covers
device exp/log ulps and per-geometry scan order.  The kernels' own errors
never set it.  Measured worst analyzer ratio: see WORST_ANALYZER_RATIO below
and docs/design/native-queue-solver.md ("Oracle parity").

Cost: the module-scoped table build takes about 10 s of CPU (measured, 260
rows drawn); every test after it is one solver call.
"""

from __future__ import annotations

import math
import time
from collections import Counter

import numpy as np
import pytest

import mm1k_oracle as oracle
from test_ops_oracle import (
    BATCH_LIMITS,
    BITWISE_GEOMETRIES,
    CPU_SOLVERS,
    FINAL_TOL,
    GEOMETRIES,
    MAX_N_896,
    _set_geometry,
    assert_matches_oracle,
    oracle_errors,
    problems_of,
)
from wva_amd.ops import solve_problems
from wva_amd.ops.batched import R_FEASIBLE, R_RATE_STAR, R_REPLICAS, _solve_problems_python

SEED = 20240611
N_DRAWN = 260
SMALL_N_SHARE = 0.6  # rows with N in [1, 64]; the rest take an edge value
MAX_DROP_SHARE = 0.25
MIN_PER_KIND = 15

# worst err / (2^-53 * A) of _solve_problems_python on this table (CPU)
WORST_ANALYZER_RATIO = 338.0
C_SCALE = 1e4  # 10 x WORST_ANALYZER_RATIO, rounded up to a power of ten


def draw(n, seed):
    """tools/fuzz_parity.draw's ranges, copied so that an edit of the tool
    cannot shift this table; only the batch limit is drawn differently
    (oracle cost grows with N, and the corners of interest are elsewhere)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 12))
    p[:, 0] = 10 ** rng.uniform(-2, 3, n)  # alpha 0.01..1000 ms
    p[:, 1] = 10 ** rng.uniform(-4, 1, n)  # beta
    p[:, 2] = 10 ** rng.uniform(-2, 3, n)  # gamma
    p[:, 3] = 10 ** rng.uniform(-5, 0, n)  # delta
    p[:, 4] = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 32768, n))  # in tokens
    p[:, 5] = np.where(rng.random(n) < 0.1, 1, rng.integers(1, 8192, n))  # out tokens
    p[:, 6] = np.where(
        rng.random(n) < SMALL_N_SHARE, rng.integers(1, 65, n), rng.choice(BATCH_LIMITS, n)
    )
    p[:, 7] = np.where(
        rng.random(n) < 0.2, 0, p[:, 2] * rng.uniform(0.5, 50, n) + rng.uniform(0, 5000, n)
    )
    p[:, 8] = np.where(rng.random(n) < 0.2, 0, p[:, 0] * rng.uniform(0.8, 10, n))
    p[:, 9] = np.where(rng.random(n) < 0.8, 0, 10 ** rng.uniform(1, 4, n))  # tps
    p[:, 10] = 10 ** rng.uniform(-2, 3, n)  # total rate req/s
    p[:, 11] = rng.integers(0, 4, n)  # min replicas
    return p


def row_bound(scale):
    return FINAL_TOL + C_SCALE * 2.0**-53 * scale


def build_wide_cases():
    started = time.perf_counter()
    rows = draw(N_DRAWN, SEED)
    cases, reasons = [], Counter()
    for row in rows:
        case, reason = oracle.oracle_solve(row)
        if case is None:
            reasons[reason] += 1
            continue
        if case["feasible"]:
            case["final_tol"] = row_bound(case["scale"])
            if case["rate_tol"] is None:  # lam is a cap: known exactly
                case["rate_tol"] = case["final_tol"]
        cases.append(case)
    dropped = sum(reasons.values())
    print(
        f"wide oracle table: {len(cases)} of {N_DRAWN} rows kept in "
        f"{time.perf_counter() - started:.1f} s; dropped {dropped}: {dict(reasons)}"
    )

    assert dropped <= MAX_DROP_SHARE * N_DRAWN, f"{dropped} of {N_DRAWN} rows dropped"
    assert 200 <= len(cases) < 512  # below 512 the auto pick is the speculative geometry
    assert sum(c["N"] <= 64 for c in cases) * 2 >= len(cases)
    feasible = [c for c in cases if c["feasible"]]
    counts = {
        "ttft-bound": sum(c["bound"] == "ttft" for c in feasible),
        "itl-bound": sum(c["bound"] == "itl" for c in feasible),
        "at a cap": sum(c["bound"] in ("tps", "none") for c in feasible),
        "above target": sum(c["has_above"] for c in feasible),
        "infeasible": len(cases) - len(feasible),
    }
    print(f"wide oracle table coverage: {counts}")
    for what, count in counts.items():
        assert count >= MIN_PER_KIND, f"only {count} rows {what}"
    return cases


@pytest.fixture(scope="module")
def wide_cases():
    return build_wide_cases()


def _fits_896(cases):
    return [c for c in cases if c["N"] <= MAX_N_896]


def test_wide_table_spans_the_claimed_ranges(wide_cases):
    p = problems_of(wide_cases)
    assert p[:, 0].min() < 0.1 and p[:, 0].max() > 100  # alpha
    assert p[:, 1].min() < 1e-3 and p[:, 1].max() > 1  # beta
    assert p[:, 4].max() > 16384 and (p[:, 4] == 0).any()  # in tokens
    assert p[:, 5].max() > 4096 and (p[:, 5] == 1).any()  # out tokens
    assert {c["N"] for c in wide_cases} >= {1, 64, 65, 257, 657, 700}


def test_c_scale_comes_from_the_analyzer(wide_cases):
    """C_SCALE is derived, not chosen: 10x the analyzer's worst scaled
    error on this table, rounded up to a power of ten.  The analyzer must
    therefore stay within a tenth of every row bound's scaled part."""
    assert C_SCALE == 10.0 ** math.ceil(math.log10(10.0 * WORST_ANALYZER_RATIO))
    worst, problems = oracle_errors(_solve_problems_python(problems_of(wide_cases)), wide_cases)
    print(f"analyzer worst err / (2^-53 A): {worst['scaled']:.3g}")
    assert not problems
    assert worst["scaled"] <= C_SCALE / 10.0


@pytest.mark.parametrize("solver", CPU_SOLVERS)
def test_wide_table_cpu(solver, wide_cases):
    assert_matches_oracle(solver(problems_of(wide_cases)), wide_cases, "cpu wide")


@pytest.mark.gpu
class TestGPUWideAgainstOracle:
    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_wide_table(self, threads, wide_cases, monkeypatch):
        _set_geometry(monkeypatch, threads)
        table = _fits_896(wide_cases) if threads == "896" else wide_cases
        problems = problems_of(table)
        assert len(problems) < 512  # auto must pick the speculative geometry
        got = solve_problems(problems, device="cuda")
        assert_matches_oracle(got, table, f"gpu wide {threads or 'auto'}")

    def test_chip_filling_auto_launch(self, wide_cases, monkeypatch):
        _set_geometry(monkeypatch, None)
        tiled = wide_cases * -(-512 // len(wide_cases))
        assert len(tiled) >= 512  # auto picks the 128-thread dual geometry
        got = solve_problems(problems_of(tiled), device="cuda")
        assert_matches_oracle(got, tiled, "gpu wide auto B>=512")

    def test_speculative_search_same_walk_as_sequential(self, wide_cases, monkeypatch):
        """As test_ops_oracle.py's test of the same name, on the wide table:
        64, 128, 384 and 896 must take the same decision walk — identical
        feasibility and replicas, rate_star within the evaluation error of
        the two sides, twice the row's bound, for binding targets too."""
        table = _fits_896(wide_cases)
        problems = problems_of(table)
        got = {}
        for threads in BITWISE_GEOMETRIES:
            _set_geometry(monkeypatch, threads)
            got[threads] = solve_problems(problems, device="cuda")
        ref = got["64"]
        feas = np.array([c["feasible"] for c in table])
        bound = np.array([c["final_tol"] for c in table if c["feasible"]])
        np.testing.assert_array_equal(ref[:, R_FEASIBLE], feas.astype(np.float64))
        for threads in BITWISE_GEOMETRIES[1:]:
            out = got[threads]
            np.testing.assert_array_equal(out[:, R_FEASIBLE], ref[:, R_FEASIBLE])
            np.testing.assert_array_equal(out[:, R_REPLICAS], ref[:, R_REPLICAS])
            diff = np.abs(out[feas, R_RATE_STAR] / ref[feas, R_RATE_STAR] - 1.0)
            print(f"rate_star {threads} vs 64: worst {(diff / bound).max():.3g} x row bound")
            assert (diff <= 2 * bound).all(), f"{threads} vs 64"
