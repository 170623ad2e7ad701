"""One row contract for every sizing implementation.

csrc/queue_core.h (``row_valid``) and ops/batched.py (``valid_rows``) state
which problem rows are valid; an invalid row must come back as the all-zero
result row from the Python analyzer path, both host bindings and every
gfx950 geometry — quietly, with the valid rows around it still solved
exactly as the oracle (tests/mm1k_oracle.py) says.  The semantic reference
is the analyzer's ``check()`` methods.
"""

from __future__ import annotations

import warnings

import numpy as np
import pytest

from fixtures import make_system, server_spec
from test_ops_oracle import (
    CPU_SOLVERS,
    GEOMETRIES,
    _set_geometry,
    assert_matches_oracle,
    cases_for_limit,
    problems_of,
)
from wva_amd.config import ModelTarget
from wva_amd.ops import BatchedAllocationSolver, solve_problems
from wva_amd.ops.batched import (
    P_ALPHA,
    P_BETA,
    P_DELTA,
    P_GAMMA,
    P_IN_TOKENS,
    P_MAX_BATCH,
    P_MIN_REPLICAS,
    P_OUT_TOKENS,
    P_TARGET_ITL,
    P_TARGET_TPS,
    P_TARGET_TTFT,
    PROBLEM_FIELDS,
    R_FEASIBLE,
    R_REPLICAS,
    _solve_problems_python,
    valid_rows,
)

BASE_ROW = (4.137, 0.027, 5.2, 0.0011, 512.0, 128.0, 64.0, 0.0, 0.0, 0.0, 10.0, 1.0)

# (field, value): BASE_ROW with this one field changed breaks the contract
INVALID_EDITS = (
    (P_OUT_TOKENS, 0.0),
    (P_OUT_TOKENS, 0.5),  # truncates to 0
    (P_OUT_TOKENS, -3.0),
    (P_OUT_TOKENS, 2.0**31),  # does not fit an int
    (P_IN_TOKENS, -5.0),
    (P_IN_TOKENS, -0.5),  # in_tokens >= 0 is tested before truncation
    (P_TARGET_TTFT, -1.0),
    (P_TARGET_ITL, -1.0),
    (P_TARGET_TPS, -1.0),
    (P_ALPHA, -1.0),
    (P_BETA, -0.01),
    (P_GAMMA, -1.0),
    (P_DELTA, -1e-4),
    (P_MAX_BATCH, 0.0),
    (P_MAX_BATCH, 0.9),  # truncates to 0
    (P_MAX_BATCH, -64.0),
    (P_MAX_BATCH, 195225787.0),  # 11 * N overflows an int
    (P_MAX_BATCH, 1e300),
) + tuple(
    (field, value)
    for field in range(PROBLEM_FIELDS)
    for value in (float("nan"), float("inf"), float("-inf"))
)

VALID_LIMITS = (2, 65)  # one wave and several: cheap for the oracle, fit every geometry


def invalid_rows():
    rows = np.tile(np.array(BASE_ROW), (len(INVALID_EDITS), 1))
    for row, (field, value) in zip(rows, INVALID_EDITS):
        row[field] = value
    return rows


@pytest.fixture(scope="module")
def interleaved():
    """(problems, valid cases, mask of the valid rows): two invalid rows
    after every valid one, so every launch and every OpenMP chunk mixes them."""
    cases = [c for n in VALID_LIMITS for c in cases_for_limit(n)]
    bad = invalid_rows()
    assert len(cases) * 2 >= len(bad)
    rows, is_valid = [], []
    for i, c in enumerate(cases):
        rows.append(c["row"])
        is_valid.append(True)
        for b in bad[2 * i : 2 * i + 2]:
            rows.append(b)
            is_valid.append(False)
    is_valid = np.array(is_valid)
    assert (~is_valid).sum() == len(bad)
    return np.stack(rows), cases, is_valid


def check_interleaved(out, interleaved, label):
    problems, cases, is_valid = interleaved
    assert out.shape == (len(problems), 6)
    bad = out[~is_valid]
    wrong = [
        (INVALID_EDITS[i], row.tolist()) for i, row in enumerate(bad) if not (row == 0.0).all()
    ]
    assert not wrong, f"{label}: invalid rows not all-zero: {wrong[:4]}"
    assert_matches_oracle(out[is_valid], cases, label)


def test_the_predicate_itself(interleaved):
    problems, _, is_valid = interleaved
    np.testing.assert_array_equal(valid_rows(problems), is_valid)
    assert valid_rows(np.array([BASE_ROW])).all()


@pytest.mark.parametrize("solver", CPU_SOLVERS)
class TestCPURowContract:
    def test_invalid_rows_are_zero_rows(self, solver, interleaved):
        with warnings.catch_warnings(), np.errstate(divide="raise", invalid="raise"):
            warnings.simplefilter("error")
            out = solver(interleaved[0])
        check_interleaved(out, interleaved, "cpu")

    def test_fractional_fields_truncate(self, solver):
        """in_tokens and min_replicas truncate toward zero, as int() does in
        the Python path: the result is bit-equal to the truncated row's, and
        no replica count is fractional."""
        rows = np.tile(np.array(BASE_ROW), (4, 1))
        rows[0, P_IN_TOKENS], rows[1, P_IN_TOKENS] = 100.6, 100.0
        rows[2, P_MIN_REPLICAS], rows[3, P_MIN_REPLICAS] = 2.5, 2.0
        out = solver(rows)
        assert (out[:, R_FEASIBLE] == 1.0).all()
        np.testing.assert_array_equal(out[0], out[1])
        np.testing.assert_array_equal(out[2], out[3])
        assert out[2, R_REPLICAS] == 2.0
        python = _solve_problems_python(rows)
        np.testing.assert_array_equal(out[:, R_REPLICAS], python[:, R_REPLICAS])


@pytest.mark.parametrize("field", ["itl", "ttft", "tps"])
def test_negative_slo_target_yields_no_allocation(field):
    """A negative SLO in a service class reaches the solvers unvalidated.
    The analyzer rejects the target, so System.calculate() allocates
    nothing for the servers of that class; the batched path must not size
    them as if they had no SLO."""
    servers = [
        server_spec("a:ns", arrival_rate=600.0),
        server_spec("c:ns", class_name="Freemium", arrival_rate=90.0),
    ]
    systems = []
    for _ in range(2):
        system, _ = make_system(servers=servers)
        target = ModelTarget(model="llama-8b", slo_itl=20.0, slo_ttft=2000.0)
        setattr(target, f"slo_{field}", -1.0)
        system.service_class("Premium").add_model_target(target)
        systems.append(system)
    scalar, batched = systems
    scalar.calculate()
    BatchedAllocationSolver().calculate(batched)
    assert scalar.server("a:ns").all_allocations == {}
    assert batched.server("a:ns").all_allocations == {}
    # the other class is untouched
    assert scalar.server("c:ns").all_allocations
    assert set(batched.server("c:ns").all_allocations) == set(
        scalar.server("c:ns").all_allocations
    )


@pytest.mark.gpu
class TestGPURowContract:
    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_invalid_rows_are_zero_rows(self, threads, interleaved, monkeypatch):
        _set_geometry(monkeypatch, threads)
        out = solve_problems(interleaved[0], device="cuda")
        check_interleaved(out, interleaved, f"gpu {threads or 'auto'}")

    def test_too_small_hint_yields_zero_rows(self, monkeypatch):
        """max_k_hint sizes the LDS table of the launch.  With the hint of
        N = 64 (704 states), rows of N = 65 (715 states) do not fit: the
        kernel's row guard must return the zero row for them instead of
        letting build_cum write past cum, and the N = 64 rows beside them
        must be unharmed.  (11 doubles past cum still lie inside this
        launch's own LDS allocation, so a missing guard shows as wrong
        results here, never as a fault.)"""
        import torch

        from wva_amd.ops import get_native

        _set_geometry(monkeypatch, None)
        fit = [c for c in cases_for_limit(64) if c["feasible"]]
        too_long = [c for c in cases_for_limit(65) if c["feasible"]]
        n = min(len(fit), len(too_long))
        assert n >= 8
        rows, fits = [], []
        for a, b in zip(fit[:n], too_long[:n]):
            rows += [a["row"], b["row"]]
            fits += [True, False]
        fits = np.array(fits)
        problems = np.stack(rows)
        assert set(problems[fits, P_MAX_BATCH]) == {64.0}
        assert set(problems[~fits, P_MAX_BATCH]) == {65.0}
        out = get_native().solve_allocations(torch.from_numpy(problems).cuda(), 704).cpu().numpy()
        assert (out[~fits] == 0.0).all()
        assert_matches_oracle(out[fits], fit[:n], "gpu hint 704")
