"""The compact-table solve (max batch N beyond 700) against the exact oracle.

The full-table kernels keep ``K = 11 * N`` doubles in LDS and stop at N = 700.
The compact form (csrc/queue_core.h, "Compact table") keeps ``cum[0..N-1]``
and takes everything past N in closed form; it is the same model, so it is
held to the same oracle (tests/mm1k_oracle.py) with the same tolerances as
test_ops_oracle.py — ``FINAL_TOL`` and ``2e-6 * cond + 1e-9`` for a binding
``rate_star`` — and nothing wider.

The table
---------
Built like test_ops_oracle.py's (its ``_Point`` and ``_case`` are reused): the
three ``SHAPES``, all seven ``KINDS``, targets that are oracle values at chosen
rates, replica quotients at m + 0.5.  N covers 701; 716, the first N no
full-table geometry fits; 767..769 and 1023..1025, where the N + 1 swept states
end on the 256- and 512-wide strides of the sweep; 2048, 4096; and 7680, the
limit.  One thing differs above 700: at 0.97 of the rate range the wait is
under float64's ``resp - serv`` cancellation floor (wait/serv 1.5e-4 at
N = 1024, below 1e-7 from 2048 on), so the TTFT target is taken at 0.999, where
wait/serv is 0.39 .. 0.01.  Ill-conditioned cases are dropped when the table is
built, from oracle quantities only (``_Point.usable``); the builder asserts how
few that is and what must survive.

For the direct ``submit_compact`` / ``solve_allocations_compact`` tests the
table also holds test_ops_oracle.py's own cases at N = 1, 2, 64, 255, 256, 257
and 700: the compact guard and sweep must be right below the old limit too.

Cost: the table builds in about 25 s of CPU, nearly all of it the oracle's
N = 4096 and N = 7680 evaluations (0.08 s each at K = 84 480 states); it is
built once per module.  Every GPU test is one to a few launches.
"""

from __future__ import annotations

import contextlib
import time
import warnings
from decimal import Decimal

import numpy as np
import pytest

import mg1_oracle
import mm1k_oracle as oracle
import wva_amd.ops as ops
import wva_amd.ops.batched as B
from test_ops_oracle import (
    ALPHA,
    BETA,
    DELTA,
    FINAL_TOL,
    GAMMA,
    KINDS,
    LAM_KNOWN_KINDS,
    MIN_REPLICAS_ABOVE,
    SHAPES,
    _case,
    _Point,
    assert_matches_oracle,
    cases_for_limit,
    problems_of,
)
from test_ops_mg1_oracle import ONE_ROW
from test_ops_oracle_wide import row_bound
from test_ops_row_contract import INVALID_EDITS, invalid_rows
from wva_amd.ops import native_available, native_cpu_available, solve_problems
from wva_amd.ops.batched import (
    P_MAX_BATCH,
    P_MIN_REPLICAS,
    P_TARGET_ITL,
    P_TARGET_TPS,
    P_TARGET_TTFT,
    P_TOTAL_RATE,
    R_FEASIBLE,
    R_RATE_STAR,
    R_REPLICAS,
    R_TTFT,
)

D = Decimal

LARGE_LIMITS = (701, 716, 767, 768, 769, 1023, 1024, 1025, 2048, 4096, 7680)
SMALL_LIMITS = (1, 2, 64, 255, 256, 257, 700)  # below the old limit, compact all the same
COMPACT_LIMIT = 7680
OLD_LIMIT = 700

ITL_FRACTIONS = (0.3, 0.8, 0.97)
TTFT_FRACTION = 0.999  # module docstring: 0.97 is under the cancellation floor here
MAX_DROP_SHARE = 0.25
MIN_WAIT_BOUND = 6  # "ttft" or "both" cases that must survive above 700
NEEDED_PER_LIMIT = ("itl", "tps", "none", "above", "below")

BAD_SCV = (float("nan"), float("inf"), float("-inf"), -0.5, -1.0)


def _large_row(in_tokens, out_tokens, n):
    row = np.zeros(12, dtype=np.float64)
    row[:7] = (ALPHA, BETA, GAMMA, DELTA, in_tokens, out_tokens, n)
    return row


def large_cases_for_limit(n, tally):
    """The constructed cases of one N > 700; ``tally`` counts the binding
    candidates tried and dropped."""
    cases = []
    for si, (in_tokens, out_tokens) in enumerate(SHAPES):
        row = _large_row(in_tokens, out_tokens, n)
        lam_min, lam_max = oracle.rate_range(row)
        pts = {f: _Point(row, f) for f in ITL_FRACTIONS + (TTFT_FRACTION,)}

        def with_targets(ttft=0.0, itl=0.0, tps=0.0):
            r = row.copy()
            r[P_TARGET_TTFT], r[P_TARGET_ITL], r[P_TARGET_TPS] = float(ttft), float(itl), tps
            return r

        def binding(name, f):
            tally["tried"] += 1
            pt = pts[f]
            if not pt.usable[name]:
                tally["dropped"] += 1  # ill-conditioned: dropped here, at construction
                return None
            return pt

        for f in ITL_FRACTIONS:
            pt = binding("itl", f)
            if pt is not None:
                cases.append(_case(with_targets(itl=pt.at.itl), "itl", n, pt.lam,
                                   2e-6 * pt.cond["itl"] + 1e-9))
        pt = binding("ttft", TTFT_FRACTION)
        if pt is not None:
            tol = 2e-6 * pt.cond["ttft"] + 1e-9
            r = with_targets(ttft=pt.at.ttft)
            cases.append(_case(r, "ttft", n, pt.lam, tol))
            if si == 0:
                cases.append(_case(r, "ttft", n, pt.lam, tol, min_replicas=MIN_REPLICAS_ABOVE))
        # both targets within the range; the one at the lower rate binds
        tally["tried"] += 1
        a, b = pts[TTFT_FRACTION], pts[0.97]
        if a.usable["ttft"] and b.usable["itl"]:
            assert b.lam < a.lam
            cases.append(_case(with_targets(ttft=a.at.ttft, itl=b.at.itl), "both", n, b.lam,
                               2e-6 * b.cond["itl"] + 1e-9))
        else:
            tally["dropped"] += 1

        top = oracle.evaluate(row, lam_max)
        bottom = oracle.evaluate(row, lam_min)
        cases.append(
            _case(with_targets(itl=bottom.itl / 2), "below", n, None, None, feasible=False)
        )
        if si == 0:  # the kinds without a bisection take one path for every shape
            cases.append(_case(with_targets(tps=1000.0), "tps", n, lam_max * D("0.9"), FINAL_TOL))
            cases.append(_case(with_targets(), "none", n, lam_max, FINAL_TOL))
            cases.append(_case(with_targets(), "none", n, lam_max, FINAL_TOL,
                               min_replicas=MIN_REPLICAS_ABOVE))
            cases.append(
                _case(with_targets(ttft=2 * top.ttft, itl=2 * top.itl), "above", n, lam_max,
                      FINAL_TOL)
            )
            cases.append(
                _case(with_targets(ttft=bottom.ttft / 2), "below", n, None, None, feasible=False)
            )
    return cases


@contextlib.contextmanager
def _memoised_evaluate():
    """While the table is built, one oracle evaluation per (model, rate): a
    target's rate is evaluated again by every case that uses it, and at these
    N an evaluation is tens of milliseconds.  Same values, restored on exit."""
    real, seen = oracle.evaluate, {}

    def evaluate(row, lam):
        key = (np.asarray(row[:7], dtype=np.float64).tobytes(), D(lam))
        hit = seen.get(key)
        if hit is None:
            hit = seen[key] = real(row, lam)
        return hit

    oracle.evaluate = evaluate
    try:
        yield
    finally:
        oracle.evaluate = real


def build_large_cases():
    started = time.perf_counter()
    tally = {"tried": 0, "dropped": 0}
    with _memoised_evaluate():
        cases = [c for n in LARGE_LIMITS for c in large_cases_for_limit(n, tally)]
    print(f"large-N table: {len(cases)} cases, {tally['dropped']} of {tally['tried']} binding "
          f"candidates dropped, built in {time.perf_counter() - started:.1f} s")
    assert tally["dropped"] <= MAX_DROP_SHARE * tally["tried"], tally
    have = {(c["N"], c["kind"]) for c in cases}
    for n in LARGE_LIMITS:
        for kind in NEEDED_PER_LIMIT:
            assert (n, kind) in have, f"no case left for N={n}, kind={kind}"
    wait_bound = sum(c["kind"] in ("ttft", "both") for c in cases)
    assert wait_bound >= MIN_WAIT_BOUND, f"only {wait_bound} ttft/both cases above {OLD_LIMIT}"
    assert {c["kind"] for c in cases} == set(KINDS)
    assert len(cases) < 512
    return cases


@pytest.fixture(scope="module")
def large_cases():
    return build_large_cases()


@pytest.fixture(scope="module")
def small_cases():
    """test_ops_oracle.py's own construction at the N the compact solve must
    also get right below the old limit."""
    return [c for n in SMALL_LIMITS for c in cases_for_limit(n)]


@pytest.fixture(scope="module")
def all_cases(large_cases, small_cases):
    return small_cases + large_cases


def _torch_free_compact(problems, scv=None):
    native = ops.get_native_cpu()
    if scv is None:
        return native.solve_allocations_compact(problems)
    return native.solve_allocations_compact(problems, scv)


def _torch_compact(problems, scv=None):
    import torch

    native = ops.get_native()
    if scv is None:
        return native.solve_allocations_compact(torch.from_numpy(problems)).numpy()
    return native.solve_allocations_compact(
        torch.from_numpy(problems), torch.from_numpy(scv)).numpy()


def _torch_free_full(problems):
    return ops.get_native_cpu().solve_allocations(problems)


def _torch_full(problems):
    import torch

    return ops.get_native().solve_allocations(torch.from_numpy(problems)).numpy()


_needs_torch_free = pytest.mark.skipif(
    not native_cpu_available(), reason="torch-free extension not built")
_needs_torch = pytest.mark.skipif(not native_available(), reason="native extension not built")

COMPACT_CPU = [
    pytest.param(_torch_free_compact, id="torch_free", marks=_needs_torch_free),
    pytest.param(_torch_compact, id="torch", marks=_needs_torch),
]
COMPACT_AND_FULL_CPU = [
    pytest.param((_torch_free_compact, _torch_free_full), id="torch_free",
                 marks=_needs_torch_free),
    pytest.param((_torch_compact, _torch_full), id="torch", marks=_needs_torch),
]


# ---------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------

def test_large_table_covers_what_it_claims(large_cases):
    # build_large_cases asserted the drop share and the per-N coverage
    assert {c["N"] for c in large_cases} == set(LARGE_LIMITS)
    assert min(LARGE_LIMITS) == OLD_LIMIT + 1 and max(LARGE_LIMITS) == COMPACT_LIMIT
    assert B.GPU_COMPACT_MAX_BATCH_LIMIT == COMPACT_LIMIT and B.GPU_MAX_BATCH_LIMIT == OLD_LIMIT
    shapes = {(c["row"][4], c["row"][5]) for c in large_cases}
    assert shapes == {(float(i), float(o)) for i, o in SHAPES}
    assert sum(c["feasible"] and c["replicas"] == int(MIN_REPLICAS_ABOVE)
               for c in large_cases) >= len(LARGE_LIMITS)


@pytest.mark.parametrize("solver", COMPACT_CPU)
def test_compact_cpu_against_oracle(solver, all_cases):
    assert_matches_oracle(solver(problems_of(all_cases)), all_cases, "cpu compact")


@pytest.mark.parametrize("solvers", COMPACT_AND_FULL_CPU)
def test_compact_agrees_with_full_table_below_the_old_limit(solvers, small_cases):
    """Two evaluations of one model: same decisions, and every value within
    the evaluation error of the two sides, 2 * FINAL_TOL; a bisected
    ``rate_star`` within the bound each side has against the oracle."""
    compact, full = solvers
    problems = problems_of(small_cases)
    got, ref = compact(problems), full(problems)
    np.testing.assert_array_equal(got[:, R_FEASIBLE], ref[:, R_FEASIBLE])
    np.testing.assert_array_equal(got[:, R_REPLICAS], ref[:, R_REPLICAS])
    worst = 0.0
    for g, r, c in zip(got, ref, small_cases):
        if not c["feasible"]:
            assert (g == 0.0).all() and (r == 0.0).all()
            continue
        # TTFT against ttft + serv, as oracle_errors does: a decode-only
        # TTFT is the bare wait, which may be zero
        scale = r[2:].copy()
        scale[R_TTFT - 2] = float(c["final"].ttft + c["final"].serv)
        rel = np.abs(g[2:] - r[2:]) / scale
        bound = np.full(4, 2 * FINAL_TOL)
        if c["kind"] not in LAM_KNOWN_KINDS:
            bound[R_RATE_STAR - 2] = c["rate_tol"]
        else:
            worst = max(worst, rel[0])
        worst = max(worst, rel[1:].max())
        assert (rel <= bound).all(), f"N={c['N']} {c['kind']}: {rel} > {bound}"
    print(f"compact vs full table, N <= {OLD_LIMIT}: worst {worst:.3g}")


@pytest.mark.parametrize("solver", COMPACT_CPU)
def test_compact_invalid_rows_are_zero_rows(solver, small_cases):
    """One invalid row per rule of the contract, two after every valid row."""
    bad = invalid_rows()
    valid = [c for c in small_cases if c["N"] in (2, 257)]
    assert len(valid) * 2 >= len(bad)
    rows, is_valid = [], []
    for i, c in enumerate(valid):
        rows.append(c["row"])
        is_valid.append(True)
        for b in bad[2 * i: 2 * i + 2]:
            rows.append(b)
            is_valid.append(False)
    is_valid = np.array(is_valid)
    assert (~is_valid).sum() == len(INVALID_EDITS)
    with warnings.catch_warnings(), np.errstate(divide="raise", invalid="raise"):
        warnings.simplefilter("error")
        out = solver(np.stack(rows))
    assert (out[~is_valid] == 0.0).all()
    assert_matches_oracle(out[is_valid], valid, "cpu compact, interleaved")


@pytest.mark.parametrize("bad", BAD_SCV, ids=[str(b) for b in BAD_SCV])
@pytest.mark.parametrize("solver", COMPACT_CPU)
def test_compact_invalid_scv_gives_the_zero_row(solver, bad, large_cases):
    row = next(c["row"] for c in large_cases if c["N"] == 701 and c["kind"] == "none")
    problems = np.stack([row] * 3)
    alone = solver(row[None, :], np.array([1.0]))[0]
    assert alone[R_FEASIBLE] == 1.0
    got = solver(problems, np.array([1.0, bad, 1.0]))
    assert np.isfinite(got).all()
    assert (got[1] == 0.0).all()
    np.testing.assert_array_equal(got[0], alone)
    np.testing.assert_array_equal(got[2], alone)


def test_compact_empty_batch_cpu():
    for solver in (_torch_free_compact, _torch_compact):
        assert solver(np.zeros((0, 12))).shape == (0, 6)


def _mixed_problems(large_cases, small_cases):
    """Rows within the old limit, rows for the compact kernel, one N = 8000
    row past it, interleaved."""
    small = [c for c in small_cases if c["N"] in (2, 64, 700)]
    middle = [c for c in large_cases if c["N"] in (701, 1024, 7680)]
    beyond = next(c["row"] for c in large_cases if c["N"] == 7680 and c["kind"] == "none").copy()
    beyond[P_MAX_BATCH] = 8000.0
    rows, where = [], []
    for i in range(max(len(small), len(middle))):
        for tag, group in (("small", small), ("middle", middle)):
            if i < len(group):
                rows.append(group[i]["row"])
                where.append(tag)
        if i == 3:
            rows.append(beyond)
            where.append("beyond")
    where = np.array(where)
    assert (where == "beyond").sum() == 1
    return np.stack(rows), where, small, middle


def test_large_n_changes_nothing_on_the_cpu(large_cases, small_cases, monkeypatch):
    problems, _, _, _ = _mixed_problems(large_cases, small_cases)
    monkeypatch.delenv("WVA_GPU_LARGE_N", raising=False)
    want = _torch_free_full(problems) if native_cpu_available() else _torch_full(problems)
    np.testing.assert_array_equal(solve_problems(problems, device="cpu"), want)
    np.testing.assert_array_equal(solve_problems(problems, device="cpu", large_n=False), want)
    np.testing.assert_array_equal(solve_problems(problems, device="cpu", large_n=True), want)
    monkeypatch.setenv("WVA_GPU_LARGE_N", "1")
    np.testing.assert_array_equal(solve_problems(problems, device="cpu"), want)
    np.testing.assert_array_equal(solve_problems(problems), want)


def test_opt_in_is_read_per_call(monkeypatch):
    monkeypatch.delenv("WVA_GPU_GRAPH", raising=False)
    monkeypatch.delenv("WVA_GPU_LARGE_N", raising=False)
    assert not B._large_n_requested(None) and B._large_n_requested(True)
    monkeypatch.setenv("WVA_GPU_LARGE_N", "1")
    assert B._large_n_requested(None) and not B._large_n_requested(False)
    monkeypatch.setenv("WVA_GPU_GRAPH", "1")  # the hipGraph route keeps the CPU split
    assert not B._large_n_requested(None) and not B._large_n_requested(True)


# ---------------------------------------------------------------------------
# gfx950: the compact-table kernel through submit_compact / collect
# ---------------------------------------------------------------------------

# one N = 1024 row whose TTFT target is wait-bound, sized under three cs^2
SCV_THREE = (0.0, 1.0, 4.0)


SCV_FRACTION = 0.995  # wait/serv 0.08 at N = 1024, and clear of the cap at lam_max


@pytest.fixture(scope="module")
def scv_cases():
    """The same N = 1024 row solved by the scaled oracle (tests/mg1_oracle.py)
    under three cs^2: three rates, three replica counts.  The TTFT target is
    the Markovian oracle's at SCV_FRACTION of the rate range — not 0.999,
    where the oracle's own margin against the lam_max cap drops the row."""
    row = _large_row(512, 128, 1024)
    pt = _Point(row, SCV_FRACTION)
    row[P_TARGET_TTFT] = float(pt.at.ttft)
    row[P_TOTAL_RATE] = float(D("2000.5") * pt.at.throughput * 1000)
    row[P_MIN_REPLICAS] = 1.0
    cases = []
    for scv in SCV_THREE:
        case, reason = mg1_oracle.oracle_solve(row, scv)
        assert case is not None and case["feasible"] and case["bound"] == "ttft", reason
        cases.append(case)
    assert len({c["replicas"] for c in cases}) == 3
    return cases


SMALL_SCV = (0.5, 2.0)


@pytest.fixture(scope="module")
def small_scv_cases():
    """test_ops_mg1_oracle.py's wait-bound N = 16 row under two cs^2 that the
    compact rows do not use; its answer moves with the scaling."""
    cases = []
    for scv in SMALL_SCV:
        case, reason = mg1_oracle.oracle_solve(ONE_ROW, scv)
        assert case is not None and case["feasible"] and case["bound"] == "ttft", reason
        case["final_tol"] = row_bound(case["scale"])  # this row's bound there too
        cases.append(case)
    assert cases[0]["replicas"] != cases[1]["replicas"]
    assert not set(SMALL_SCV) & set(SCV_THREE)
    return cases


def _scv_of(cases):
    return np.array([c["scv"] for c in cases], dtype=np.float64)


@pytest.mark.gpu
class TestGPUCompact:
    @pytest.fixture(autouse=True)
    def _pool_is_idle_afterwards(self, monkeypatch):
        monkeypatch.delenv("WVA_GPU_GRAPH", raising=False)
        monkeypatch.delenv("WVA_GPU_LARGE_N", raising=False)
        monkeypatch.delenv("WVA_GPU_THREADS", raising=False)
        yield
        assert ops.get_native().dispatch_pool_stats()[1] == 0

    @staticmethod
    def _compact(problems, max_n, scv=None):
        native = ops.get_native()
        problems = np.ascontiguousarray(problems)
        if scv is None:
            return native.collect(native.submit_compact(problems, max_n))
        return native.collect(native.submit_compact(problems, max_n, scv))

    def test_whole_table_in_one_launch(self, all_cases):
        """N = 1 and N = 7680 share one launch and one max_n."""
        got = self._compact(problems_of(all_cases), COMPACT_LIMIT)
        assert_matches_oracle(got, all_cases, "gpu compact")

    def test_row_by_row(self, all_cases):
        """B = 1 launches, each reserving exactly its own N, sixteen in
        flight at a time (a bounded slot pool)."""
        native = ops.get_native()
        got = []
        for lo in range(0, len(all_cases), 16):
            tickets = [native.submit_compact(c["row"][None, :].copy(), c["N"])
                       for c in all_cases[lo: lo + 16]]
            got += [native.collect(t) for t in tickets]
        got = np.concatenate(got)
        assert_matches_oracle(got, all_cases, "gpu compact, B = 1")

    def test_row_beyond_max_n_is_the_zero_row(self, large_cases):
        picked = [c for c in large_cases if c["N"] in (701, 1024, 1025) and c["feasible"]]
        assert {c["N"] for c in picked} == {701, 1024, 1025}
        got = self._compact(problems_of(picked), 1024)
        too_big = np.array([c["N"] > 1024 for c in picked])
        assert too_big.any() and (got[too_big] == 0.0).all()
        kept = [c for c in picked if c["N"] <= 1024]
        assert_matches_oracle(got[~too_big], kept, "gpu compact, neighbours of a refused row")

    def test_invalid_rows_and_scv_are_zero_rows(self, large_cases):
        bad = invalid_rows()
        good = next(c for c in large_cases if c["N"] == 716 and c["kind"] == "none")
        problems = np.concatenate([good["row"][None, :], bad, good["row"][None, :]])
        got = self._compact(problems, 716)
        assert (got[1:-1] == 0.0).all()
        assert_matches_oracle(got[[0, -1]], [good, good], "gpu compact around invalid rows")
        scv = np.array((1.0,) + BAD_SCV + (1.0,))
        got = self._compact(np.stack([good["row"]] * len(scv)), 716, scv)
        assert np.isfinite(got).all() and (got[1:-1] == 0.0).all()
        assert_matches_oracle(got[[0, -1]], [good, good], "gpu compact around invalid cs^2")

    def test_empty_batch(self):
        assert self._compact(np.zeros((0, 12)), 1024).shape == (0, 6)

    def test_lds_refusal_leaves_the_slot_reusable(self, large_cases):
        native = ops.get_native()
        few = [c for c in large_cases if c["N"] == 767]
        with pytest.raises(RuntimeError, match="LDS"):
            native.submit_compact(problems_of(few), 9000)
        assert native.dispatch_pool_stats()[1] == 0
        assert_matches_oracle(self._compact(problems_of(few), 767), few, "gpu after refusal")

    def test_opt_in_routing(self, large_cases, small_cases):
        problems, where, small, middle = _mixed_problems(large_cases, small_cases)
        off = solve_problems(problems, device="cuda", large_n=False)
        on = solve_problems(problems, device="cuda", large_n=True)
        np.testing.assert_array_equal(on[where == "small"], off[where == "small"])
        assert_matches_oracle(on[where == "small"], small, "gpu opt-in, N <= 700")
        assert_matches_oracle(on[where == "middle"], middle, "gpu opt-in, compact rows")
        cpu = solve_problems(problems[where == "beyond"], device="cpu")
        assert cpu[0, R_FEASIBLE] == 1.0
        np.testing.assert_array_equal(on[where == "beyond"], cpu)
        np.testing.assert_array_equal(off[where == "beyond"], cpu)

    def test_opt_in_through_the_environment(self, large_cases, small_cases, monkeypatch):
        problems, where, _, middle = _mixed_problems(large_cases, small_cases)
        calls = []
        native = ops.get_native()
        real = native.submit_compact

        def spy(*args):
            calls.append(len(args[0]))
            return real(*args)

        monkeypatch.setattr(native, "submit_compact", spy)
        solve_problems(problems, device="cuda")
        assert not calls  # off by default
        monkeypatch.setenv("WVA_GPU_LARGE_N", "1")
        on = solve_problems(problems, device="cuda")
        assert calls == [len(middle)]
        assert_matches_oracle(on[where == "middle"], middle, "gpu WVA_GPU_LARGE_N=1")
        solve_problems(problems, device="cuda", large_n=False)
        assert calls == [len(middle)]  # False forces the CPU split

    def test_three_scv_in_one_compact_launch(self, scv_cases):
        got = self._compact(problems_of(scv_cases), 1024, _scv_of(scv_cases))
        assert len(set(got[:, R_REPLICAS])) == 3
        assert_matches_oracle(got, scv_cases, "gpu compact, three cs^2")

    def test_each_part_of_a_mixed_launch_takes_its_own_scv(self, scv_cases, small_scv_cases):
        """Wait-bound small rows under cs^2 = 0.5 and 2 around compact rows
        under 0 / 1 / 4, every expectation from the scaled oracle: a part
        handed any other slice of the vector misses its replica counts."""
        cases = small_scv_cases[:1] + scv_cases + small_scv_cases[1:]
        scv = _scv_of(cases)
        assert len(set(scv)) == len(scv)
        got = solve_problems(problems_of(cases), device="cuda", scv=scv, large_n=True)
        assert_matches_oracle(got, cases, "gpu opt-in, mixed cs^2")

    def test_no_vector_after_a_vector_is_markovian(self, scv_cases):
        native = ops.get_native()
        assert native.dispatch_pool_stats()[1] == 0  # so both submits take the same slot
        problems = problems_of(scv_cases)
        markovian = next(c for c in scv_cases if c["scv"] == 1.0)
        self._compact(problems, 1024, np.full(len(problems), 4.0))
        got = self._compact(problems, 1024)
        assert_matches_oracle(got, [markovian] * len(problems), "gpu compact, stale cs^2")
