"""M/G/1-corrected sizing (per-row cs^2) against the scaled exact oracle.

The table is test_ops_oracle_wide.py's draw — the whole claimed parameter
range — with row ``i`` given the service-time cs^2 ``SCV_CYCLE[i % 5]``, each
row *solved by the oracle* under the correction (tests/mg1_oracle.py: the
unchanged ``oracle_solve`` over an evaluation whose wait is scaled by
``(1 + cs^2) / 2``).  Every implementation that takes a cs^2 vector — the
Python analyzer, the two native CPU bindings, the public ``solve_problems``
and each gfx950 kernel geometry — must match it; the same solver *without*
the vector must not, on at least ``MIN_MARKOVIAN_MISMATCHES`` rows, or the
table would not see the correction at all.

Tolerances are the wide table's, none new: feasibility and replicas exact,
``rate_star`` of a binding target ``2e-6 * cond + 1e-9``, everything else
``FINAL_TOL + C_SCALE * 2^-53 * A`` per row.  ``C_SCALE`` follows by the wide
test's own rule from the analyzer's worst scaled error *with the vector* on
this table (measured on CPU: 337.9, so 1e4 again), and the derivation is
asserted below.

Measured when written (CPU): 13 of 260 rows dropped
(``replica_quotient_on_integer`` 9, ``target_ties_with_cap`` 4), 247 kept:
103 TTFT-bound, 33 ITL-bound, 59 at a cap, 52 infeasible.  A solver that
ignores the vector mismatches 128 of the 247, 30 of them in the replica count.

Also here: the cs^2 part of the row contract (NaN, +-inf, negative values and
the unresolved -1 sentinel give the all-zero row; a wrong-length or
non-float64 vector raises), bit-identity of "no vector", scalar 1.0 and a
vector of ones, and on the GPU the paths a vector can get lost on: row
indexing, the oversized-N split to the CPU, hipGraph replay, slot reuse and
two launches in flight.

Cost: the module-scoped table build takes about 10 s of CPU; every test after
it is one solver call.
"""

from __future__ import annotations

import math
import time
from collections import Counter

import numpy as np
import pytest

import mg1_oracle
import mm1k_oracle
import test_ops_oracle_wide as wide
import wva_amd.ops as ops
import wva_amd.ops.batched as B
from test_ops_oracle import (
    GEOMETRIES,
    MAX_N_896,
    _set_geometry,
    assert_matches_oracle,
    oracle_errors,
    problems_of,
)
from wva_amd.ops import native_available, native_cpu_available, solve_problems
from wva_amd.ops.batched import (
    P_MAX_BATCH,
    R_FEASIBLE,
    R_RATE_STAR,
    R_REPLICAS,
    _solve_problems_python,
    valid_scv,
)

SCV_CYCLE = (0.0, 0.25, 0.5, 2.0, 4.0)
MAX_DROP_SHARE = 0.25
MIN_PER_KIND = 15
MIN_MARKOVIAN_MISMATCHES = 100

# worst err / (2^-53 * A) of _solve_problems_python, given the cs^2 vector,
# on this table (CPU; measured 337.9)
WORST_ANALYZER_RATIO = 338.0
C_SCALE = 1e4  # 10 x WORST_ANALYZER_RATIO, rounded up to a power of ten

# cs^2 values no row may carry; -1 is the unresolved "use the fleet value"
BAD_SCV = (float("nan"), float("inf"), float("-inf"), -0.5, -1.0)


def build_mg1_cases():
    started = time.perf_counter()
    rows = wide.draw(wide.N_DRAWN, wide.SEED)
    cases, reasons = [], Counter()
    for i, row in enumerate(rows):
        case, reason = mg1_oracle.oracle_solve(row, SCV_CYCLE[i % len(SCV_CYCLE)])
        if case is None:
            reasons[reason] += 1
            continue
        if case["feasible"]:
            case["final_tol"] = wide.row_bound(case["scale"])
            if case["rate_tol"] is None:  # lam is a cap: known exactly
                case["rate_tol"] = case["final_tol"]
        cases.append(case)
    dropped = sum(reasons.values())
    print(
        f"mg1 oracle table: {len(cases)} of {wide.N_DRAWN} rows kept in "
        f"{time.perf_counter() - started:.1f} s; dropped {dropped}: {dict(reasons)}"
    )
    assert mm1k_oracle.evaluate.__module__ == "mm1k_oracle"  # the swap was undone
    assert dropped <= MAX_DROP_SHARE * wide.N_DRAWN, f"{dropped} of {wide.N_DRAWN} rows dropped"
    assert 200 <= len(cases) < 512  # below 512 the auto pick is the speculative geometry
    feasible = [c for c in cases if c["feasible"]]
    counts = {
        "ttft-bound": sum(c["bound"] == "ttft" for c in feasible),
        "itl-bound": sum(c["bound"] == "itl" for c in feasible),
        "at a cap": sum(c["bound"] in ("tps", "none") for c in feasible),
        "infeasible": len(cases) - len(feasible),
    }
    print(f"mg1 oracle table coverage: {counts}")
    for what, count in counts.items():
        assert count >= MIN_PER_KIND, f"only {count} rows {what}"
    for scv in SCV_CYCLE:  # every cs^2 of the cycle binds a TTFT target somewhere
        assert any(c["scv"] == scv and c["bound"] == "ttft" for c in feasible), scv
    return cases


@pytest.fixture(scope="module")
def mg1_cases():
    return build_mg1_cases()


def scv_of(cases):
    return np.array([c["scv"] for c in cases], dtype=np.float64)


def _fits_896(cases):
    return [c for c in cases if c["N"] <= MAX_N_896]


# -- the CPU solvers, each as f(problems, scv=None) --------------------------

def _python(problems, scv=None):
    if scv is None:
        return _solve_problems_python(problems)
    return _solve_problems_python(problems, scv=scv)


def _torch_free(problems, scv=None):
    return ops.get_native_cpu().solve_allocations(problems, scv)


def _torch(problems, scv=None):
    import torch

    scv_t = scv if scv is None or not isinstance(scv, np.ndarray) else torch.from_numpy(scv)
    return ops.get_native().solve_allocations(torch.from_numpy(problems), -1, scv_t).numpy()


def _public(problems, scv=None):
    return solve_problems(problems, "cpu", scv=scv)


_NEEDS_TORCH_FREE = pytest.mark.skipif(
    not native_cpu_available(), reason="torch-free extension not built"
)
_NEEDS_TORCH = pytest.mark.skipif(not native_available(), reason="native extension not built")

HOST_BINDINGS = [
    pytest.param(_torch_free, id="torch_free", marks=_NEEDS_TORCH_FREE),
    pytest.param(_torch, id="torch", marks=_NEEDS_TORCH),
]
CPU_SOLVERS = [pytest.param(_python, id="python")] + HOST_BINDINGS
# ... and the public entry point, which picks the first native binding built
ALL_CPU = CPU_SOLVERS + [pytest.param(_public, id="solve_problems")]


@pytest.fixture(autouse=True)
def _markovian_environment(monkeypatch):
    """No test here depends on the environment's analyzer mode: an explicit
    vector never reads it, and ``scv=None`` must mean the Markovian model."""
    monkeypatch.delenv("WVA_ANALYZER", raising=False)
    monkeypatch.delenv("WVA_SERVICE_SCV", raising=False)


# ---------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------

def test_c_scale_comes_from_the_analyzer(mg1_cases):
    """As test_ops_oracle_wide.py: C_SCALE is 10x the analyzer's worst scaled
    error on this table — here with the cs^2 vector — rounded up to a power
    of ten, and it is the wide table's constant that the bounds use."""
    assert C_SCALE == 10.0 ** math.ceil(math.log10(10.0 * WORST_ANALYZER_RATIO))
    assert C_SCALE == wide.C_SCALE
    got = _python(problems_of(mg1_cases), scv_of(mg1_cases))
    worst, problems = oracle_errors(got, mg1_cases)
    print(f"analyzer worst err / (2^-53 A) with cs^2: {worst['scaled']:.4g}")
    assert not problems
    assert worst["scaled"] <= WORST_ANALYZER_RATIO
    assert worst["scaled"] <= C_SCALE / 10.0


@pytest.mark.parametrize("solver", ALL_CPU)
def test_mg1_table_cpu(solver, mg1_cases):
    """The test that fails without the feature: with the vector every solver
    matches the scaled oracle; without it the same solver does not."""
    problems, scv = problems_of(mg1_cases), scv_of(mg1_cases)
    assert_matches_oracle(solver(problems, scv), mg1_cases, "cpu mg1")
    _, mismatches = oracle_errors(solver(problems), mg1_cases)
    replicas = sum("replicas=" in m for m in mismatches)
    print(f"without the vector: {len(mismatches)} of {len(mg1_cases)} rows mismatch, "
          f"{replicas} in the replica count")
    assert len(mismatches) >= MIN_MARKOVIAN_MISMATCHES


# one row, three cs^2: a wait-bound (tight TTFT) problem whose answer moves
# with the scaling.  Oracle-solved once, shared.
ONE_ROW = np.array([12.0, 6.0, 4.0, 0.01, 32.0, 25.0, 16.0, 15.0, 0.0, 0.0, 200.0, 1.0])
ONE_ROW_SCV = (0.0, 1.0, 4.0)


@pytest.fixture(scope="module")
def one_row_cases():
    cases = []
    for scv in ONE_ROW_SCV:
        case, reason = mg1_oracle.oracle_solve(ONE_ROW, scv)
        assert case is not None and case["feasible"] and case["bound"] == "ttft", reason
        case["final_tol"] = wide.row_bound(case["scale"])
        cases.append(case)
    rates = [float(c["rate_star"]) for c in cases]
    assert rates[0] > rates[1] * 1.02 > rates[2] * 1.02 * 1.02  # really three answers
    assert len({c["replicas"] for c in cases}) == 3
    return cases


@pytest.mark.parametrize("solver", ALL_CPU)
def test_one_row_three_scv_cpu(solver, one_row_cases):
    got = solver(problems_of(one_row_cases), scv_of(one_row_cases))
    assert_matches_oracle(got, one_row_cases, "cpu one row, three cs^2")


# ---------------------------------------------------------------------------
# Contract
# ---------------------------------------------------------------------------

def test_valid_scv_mirrors_the_native_predicate():
    values = np.array(BAD_SCV + (0.0, 0.25, 1.0, 4.0, 1.7976931348623157e308, -0.0))
    want = np.array([False] * len(BAD_SCV) + [True] * 6)
    np.testing.assert_array_equal(valid_scv(values), want)


@pytest.mark.parametrize("bad", BAD_SCV, ids=[str(b) for b in BAD_SCV])
@pytest.mark.parametrize("solver", ALL_CPU)
def test_invalid_scv_gives_the_zero_row(solver, bad):
    """An otherwise valid row between two valid ones: only it is zeroed, and
    the neighbours' answers are those of their own cs^2."""
    problems = np.stack([ONE_ROW] * 3)
    alone = [solver(ONE_ROW[None, :], np.array([s]))[0] for s in (0.5, 2.0)]
    assert alone[0][R_FEASIBLE] == 1.0 and alone[1][R_FEASIBLE] == 1.0
    assert alone[0][R_RATE_STAR] != alone[1][R_RATE_STAR]
    with np.errstate(divide="raise", invalid="raise"):
        got = solver(problems, np.array([0.5, bad, 2.0]))
    assert np.isfinite(got).all()
    assert (got[1] == 0.0).all()
    np.testing.assert_array_equal(got[0], alone[0])
    np.testing.assert_array_equal(got[2], alone[1])


@pytest.mark.parametrize("solver", ALL_CPU)
def test_malformed_vector_raises(solver):
    problems = np.stack([ONE_ROW] * 3)
    raised = (TypeError, ValueError, RuntimeError)
    for vector in (
        np.ones(2),  # wrong length
        np.ones(4),
        np.ones((3, 1)),  # wrong rank
        np.ones(3, dtype=np.float32),  # not float64
        np.ones(3, dtype=np.int64),
    ):
        with pytest.raises(raised):
            solver(problems, vector)
    good = solver(problems, np.ones(3))
    assert (good[:, R_FEASIBLE] == 1.0).all()  # nothing was left broken


@pytest.mark.parametrize("binding", HOST_BINDINGS)
def test_non_contiguous_vector_raises(binding):
    problems = np.stack([ONE_ROW] * 3)
    strided = np.ones(6)[::2]
    assert strided.shape == (3,) and not strided.flags.c_contiguous
    if binding is _torch:
        import torch

        strided = torch.from_numpy(np.ones(6))[::2]
    with pytest.raises((TypeError, ValueError, RuntimeError)):
        binding(problems, strided)


# ---------------------------------------------------------------------------
# Identity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("binding", HOST_BINDINGS)
def test_ones_are_bit_identical_to_no_vector_cpu(binding, mg1_cases, monkeypatch):
    """``x * 1.0`` is exact and ``fma(x, 1.0, y)`` rounds ``x + y`` — checked,
    not assumed: no vector, scalar 1.0 and a vector of ones, on each host
    binding and through the public entry point routed to it."""
    problems = np.concatenate([problems_of(mg1_cases), np.stack([ONE_ROW] * 3)])
    want = binding(problems)
    assert (want[:, R_FEASIBLE] == 1.0).sum() >= 100
    np.testing.assert_array_equal(binding(problems, np.ones(len(problems))), want)
    if binding is _torch:
        monkeypatch.setattr(ops, "_native_cpu", None)  # the torch binding is second in line
    np.testing.assert_array_equal(solve_problems(problems, "cpu"), want)
    np.testing.assert_array_equal(solve_problems(problems, "cpu", scv=1.0), want)
    np.testing.assert_array_equal(
        solve_problems(problems, "cpu", scv=np.ones(len(problems))), want
    )


def test_explicit_vector_never_reads_the_environment(mg1_cases, monkeypatch):
    problems, scv = problems_of(mg1_cases), scv_of(mg1_cases)
    want = solve_problems(problems, "cpu", scv=scv)
    monkeypatch.setenv("WVA_ANALYZER", "mg1")
    monkeypatch.setenv("WVA_SERVICE_SCV", "3.0")
    np.testing.assert_array_equal(solve_problems(problems, "cpu", scv=scv), want)


@pytest.mark.skipif(
    not (native_cpu_available() or native_available()), reason="no native binding built"
)
def test_explicit_vector_stays_off_the_python_analyzer(one_row_cases, monkeypatch):
    def fail(*args, **kwargs):
        raise AssertionError("the Python analyzer was used")

    monkeypatch.setattr(B, "_solve_problems_python", fail)
    got = solve_problems(problems_of(one_row_cases), "cpu", scv=scv_of(one_row_cases))
    assert_matches_oracle(got, one_row_cases, "native, spy on the analyzer")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
class TestGPUMG1AgainstOracle:
    @pytest.fixture(autouse=True)
    def _pool_is_idle_afterwards(self):
        yield
        assert ops.get_native().dispatch_pool_stats()[1] == 0

    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_mg1_table(self, threads, mg1_cases, monkeypatch):
        _set_geometry(monkeypatch, threads)
        table = _fits_896(mg1_cases) if threads == "896" else mg1_cases
        problems = problems_of(table)
        assert len(problems) < 512  # auto must pick the speculative geometry
        got = solve_problems(problems, device="cuda", scv=scv_of(table))
        assert_matches_oracle(got, table, f"gpu mg1 {threads or 'auto'}")

    def test_chip_filling_auto_launch(self, mg1_cases, monkeypatch):
        _set_geometry(monkeypatch, None)
        tiled = mg1_cases * -(-512 // len(mg1_cases))
        assert len(tiled) >= 512  # auto picks the 128-thread dual geometry
        got = solve_problems(problems_of(tiled), device="cuda", scv=scv_of(tiled))
        assert_matches_oracle(got, tiled, "gpu mg1 auto B>=512")

    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_ones_are_bit_identical_to_no_vector(self, threads, mg1_cases, monkeypatch):
        _set_geometry(monkeypatch, threads)
        table = _fits_896(mg1_cases) if threads == "896" else mg1_cases
        problems = problems_of(table)
        want = solve_problems(problems, device="cuda")
        assert (want[:, R_FEASIBLE] == 1.0).sum() >= 100
        for scv in (1.0, np.ones(len(problems))):
            np.testing.assert_array_equal(
                solve_problems(problems, device="cuda", scv=scv), want
            )

    def test_ones_are_bit_identical_chip_filling(self, mg1_cases, monkeypatch):
        _set_geometry(monkeypatch, None)
        problems = problems_of(mg1_cases * -(-512 // len(mg1_cases)))
        assert len(problems) >= 512
        want = solve_problems(problems, device="cuda")
        for scv in (1.0, np.ones(len(problems))):
            np.testing.assert_array_equal(
                solve_problems(problems, device="cuda", scv=scv), want
            )

    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_invalid_scv_gives_the_zero_row(self, threads, monkeypatch):
        _set_geometry(monkeypatch, threads)
        good = solve_problems(np.stack([ONE_ROW] * 2), device="cuda", scv=np.array([0.5, 2.0]))
        assert (good[:, R_FEASIBLE] == 1.0).all()
        problems = np.stack([ONE_ROW] * (len(BAD_SCV) + 2))
        got = solve_problems(
            problems, device="cuda", scv=np.array((0.5,) + BAD_SCV + (2.0,))
        )
        assert np.isfinite(got).all()
        assert (got[1:-1] == 0.0).all()
        np.testing.assert_array_equal(got[[0, -1]], good)

    def test_malformed_vector_raises(self):
        native = ops.get_native()
        problems = np.stack([ONE_ROW] * 3)
        for vector in (np.ones(2), np.ones(4), np.ones(3, dtype=np.float32), np.ones(6)[::2]):
            with pytest.raises((TypeError, ValueError, RuntimeError)):
                native.submit(problems, 176, vector)
        assert native.dispatch_pool_stats()[1] == 0  # no slot was left busy

    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_one_row_three_scv(self, threads, one_row_cases, monkeypatch):
        """B = 3, the same row under three cs^2: a stride or index mistake
        in the vector gives some row another row's answer."""
        _set_geometry(monkeypatch, threads)
        got = solve_problems(
            problems_of(one_row_cases), device="cuda", scv=scv_of(one_row_cases)
        )
        assert_matches_oracle(got, one_row_cases, f"gpu one row {threads or 'auto'}")
        assert len(set(got[:, R_REPLICAS])) == 3

    def test_cpu_split_carries_the_matching_scv(self, mg1_cases, monkeypatch):
        """N = 700 stays on the GPU, N = 701 goes to the CPU: each part must
        take the cs^2 of its own rows."""
        _set_geometry(monkeypatch, None)
        at_limit = [c for c in mg1_cases if c["N"] == 700 and c["bound"] == "ttft"]
        assert len(at_limit) >= 2 and len({c["scv"] for c in at_limit}) >= 2
        rows, scv = [], []
        for c in at_limit:
            over = c["row"].copy()
            over[P_MAX_BATCH] = 701.0
            rows += [c["row"], over]
            scv += [c["scv"], SCV_CYCLE[(SCV_CYCLE.index(c["scv"]) + 2) % len(SCV_CYCLE)]]
        problems, scv = np.stack(rows), np.array(scv)
        got = solve_problems(problems, device="cuda", scv=scv)
        assert_matches_oracle(got[0::2], at_limit, "gpu part of the split")
        want_over = solve_problems(problems[1::2], device="cpu", scv=scv[1::2])
        assert (want_over[:, R_FEASIBLE] == 1.0).all()
        np.testing.assert_array_equal(got[1::2], want_over)
        # and the answers do depend on which cs^2 a row got (not on every
        # row: a TTFT target can bind through the prefill term alone, at a
        # rate where nothing waits)
        swapped = solve_problems(problems[1::2], device="cpu", scv=scv[0::2])
        assert (swapped[:, R_RATE_STAR] != want_over[:, R_RATE_STAR]).any()

    def test_hipgraph_replay_refreshes_the_vector(self, mg1_cases, monkeypatch):
        monkeypatch.setattr(B, "_graph_cache", {})
        monkeypatch.setattr(B, "_graph_disabled", False)
        monkeypatch.setenv("WVA_GPU_GRAPH", "1")
        _set_geometry(monkeypatch, None)
        table = mg1_cases[:60]
        problems, scv = problems_of(table), scv_of(table)
        other = np.roll(scv, 1)  # every row gets a different cs^2 of the cycle
        assert (other != scv).sum() >= 50
        captured = solve_problems(problems, device="cuda", scv=other)
        replayed = solve_problems(problems, device="cuda", scv=scv)
        assert len(B._graph_cache) == 1 and not B._graph_disabled
        assert_matches_oracle(replayed, table, "gpu graph replay")
        assert (captured[:, R_RATE_STAR] != replayed[:, R_RATE_STAR]).sum() >= 10
        # a launch without a vector is another graph, and Markovian
        plain = solve_problems(problems, device="cuda")
        assert len(B._graph_cache) == 2 and not B._graph_disabled
        monkeypatch.setenv("WVA_GPU_GRAPH", "0")
        np.testing.assert_array_equal(plain, solve_problems(problems, device="cuda"))

    def test_slot_reuse_without_vector_is_markovian(self, mg1_cases, monkeypatch):
        """A submit with a vector, then one without on the same slot: the
        second must not see what the first left behind the rows."""
        import torch

        _set_geometry(monkeypatch, None)
        native = ops.get_native()
        table = mg1_cases[:60]
        problems, scv = problems_of(table), scv_of(table)
        max_k = int(problems[:, P_MAX_BATCH].max()) * 11
        want = native.solve_allocations(torch.from_numpy(problems).cuda(), max_k).cpu().numpy()
        with_vector = native.collect(native.submit(problems, max_k, scv))
        slots = native.dispatch_pool_stats()[0]
        without = native.collect(native.submit(problems, max_k))
        assert native.dispatch_pool_stats() == (slots, 0)  # no slot added: the same one
        assert_matches_oracle(with_vector, table, "gpu dispatch with vector")
        np.testing.assert_array_equal(without, want)
        assert (with_vector[:, R_RATE_STAR] != without[:, R_RATE_STAR]).sum() >= 10

    def test_two_tickets_in_flight_with_different_vectors(self, mg1_cases, monkeypatch):
        _set_geometry(monkeypatch, None)
        native = ops.get_native()
        table = mg1_cases[:60]
        problems, scv = problems_of(table), scv_of(table)
        other = np.roll(scv, 1)
        max_k = int(problems[:, P_MAX_BATCH].max()) * 11
        want_other = native.collect(native.submit(problems, max_k, other))
        first = native.submit(problems, max_k, scv)
        second = native.submit(problems, max_k, other)
        assert native.dispatch_pool_stats()[1] == 2
        got_other = native.collect(second)
        got = native.collect(first)
        assert_matches_oracle(got, table, "gpu first of two tickets")
        np.testing.assert_array_equal(got_other, want_other)
        assert (got[:, R_RATE_STAR] != got_other[:, R_RATE_STAR]).sum() >= 10
