"""Sizing solvers against an exact oracle (tests/mm1k_oracle.py).

Every implementation of the sizing problem — the Python analyzer, the two
native CPU bindings and each gfx950 kernel geometry — is compared with a
50-digit evaluation of the same birth-death chain that shares no code with
them.  The cases are *constructed* from the oracle so that the answer is
known and nothing sits on a decision boundary: targets are oracle values at
chosen rates, the offered load puts the replica quotient at m + 0.5, and
badly conditioned bisections are dropped when the table is built (never
when results are compared).

Tolerances
----------
``rate_star`` of a binding TTFT/ITL target is only determined to the
bisection's 1e-6 relative stop in y, i.e. to ``1e-6 * cond`` with
``cond = |dln throughput/dln lam| / |dln y/dln lam|`` from the oracle; the
bound is ``2e-6 * cond + 1e-9``.  Everything else (final ITL, TTFT, rho, and
``rate_star`` where lam is known exactly) uses ``FINAL_TOL``: 100x the worst
error of the Python analyzer — the project's semantic reference — on this
very table, rounded up to a power of ten.  Measured worst analyzer error:
4.7e-14 (rho; rate_star 3.3e-14, TTFT 2.7e-14, ITL 1.4e-14), hence 1e-11.  The 100x covers device
exp/log ulps and per-geometry summation order, which pass through the same
``resp - serv`` cancellation.  The figures measured for every implementation
are in docs/design/native-queue-solver.md ("Oracle parity").
"""

from __future__ import annotations

import warnings
from decimal import Decimal

import numpy as np
import pytest

import mm1k_oracle as oracle
from wva_amd.ops import native_available, native_cpu_available, solve_problems
from wva_amd.ops.batched import (
    GPU_MAX_BATCH_LIMIT,
    P_MAX_BATCH,
    P_MIN_REPLICAS,
    P_TARGET_ITL,
    P_TARGET_TPS,
    P_TARGET_TTFT,
    P_TOTAL_RATE,
    R_FEASIBLE,
    R_ITL,
    R_RATE_STAR,
    R_REPLICAS,
    R_RHO,
    R_TTFT,
    _solve_problems_python,
)

FINAL_TOL = 1e-11

# every value sits on an edge: 6 -> K=66 straddles one wave; 64/384/448 land
# on exact or partial build_cum chunks for 64/384/896 threads; 255..257 on
# the 256-wide sweep; 63..65 and 127..129 on wave_lower_bound's 64-probe
# rounds; 657 is the largest N the 896 geometry fits; 700 is the GPU limit
BATCH_LIMITS = (1, 2, 6, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 448, 511, 512, 657, 700)
MAX_N_896 = 657  # 11*N + 896 + 64 <= 8192
assert BATCH_LIMITS[-1] == GPU_MAX_BATCH_LIMIT

# (in_tokens, out_tokens): mixed, decode-only, prefill-heavy
SHAPES = ((512, 128), (0, 64), (2000, 2))
# single-output-token shapes (num_decode rule / num_decode = 0) at a few N
EXTRA_SHAPES = ((0, 1), (300, 1))
EXTRA_SHAPE_LIMITS = (2, 256, 657)

# decode base, prefill base/slope (ms) and the decode slope.  The slope is
# chosen by N so that both targets can bind somewhere in the table: at tiny N
# ITL = alpha + beta * concurrency only moves with load if beta/alpha is
# large, while at large N a large beta saturates mu(b) so early that no
# queue (hence no TTFT signal) forms even at 0.97 * lam_max.
ALPHA, GAMMA, DELTA = 4.137, 5.2, 0.0011
BETA_SMALL_N, BETA = 0.413, 0.027
SMALL_N = 6

FRACTIONS = (0.3, 0.8, 0.97)
# (f of the TTFT target, f of the ITL target), in order of preference; the
# lower f binds.  TTFT is only usable near saturation at large N.
BOTH_PAIRS = ((0.8, 0.97), (0.97, 0.8), (0.97, 0.3), (0.3, 0.8))
REPLICA_M = 3  # total_rate = (m + 0.5) * rate_star  ->  exactly m + 1 replicas
MIN_REPLICAS_ABOVE = 6.0

KINDS = ("ttft", "itl", "both", "tps", "none", "above", "below")
LAM_KNOWN_KINDS = ("tps", "none", "above")  # lam_expected is exact: tight rate_star bound
# N = 1 serves one request at a time, so the mean service time is 1/mu(1)
# whatever the load and ITL does not depend on lam at all: no ITL target can
# bind there.  The builder checks this on the oracle instead of assuming it.
FLAT_ITL_CELLS = ((1, "itl"), (1, "both"))

D = Decimal
_H = D("0.0001")


def _base_row(in_tokens, out_tokens, n):
    row = np.zeros(12, dtype=np.float64)
    beta = BETA_SMALL_N if n <= SMALL_N else BETA
    row[:7] = (ALPHA, beta, GAMMA, DELTA, in_tokens, out_tokens, n)
    return row


class _Point:
    """Oracle facts at lam0 = lam_min + f * (lam_max - lam_min)."""

    def __init__(self, row, f):
        lam_min, lam_max = oracle.rate_range(row)
        self.lam = lam_min + D(f) * (lam_max - lam_min)
        self.at = oracle.evaluate(row, self.lam)
        up = oracle.evaluate(row, self.lam * (1 + _H))
        dn = oracle.evaluate(row, self.lam * (1 - _H))

        def slope(name):  # dln y / dln lam, central difference
            y = getattr(self.at, name)
            return abs((getattr(up, name) - getattr(dn, name)) / y / (2 * _H)) if y else D(0)

        thr = slope("throughput")
        self.cond, self.usable = {}, {}
        for name in ("ttft", "itl"):
            s = slope(name)
            ok = s >= D("0.001")
            if ok and name == "ttft":
                # below this the target is under float64's cancellation
                # floor of wait = resp - serv
                ok = self.at.wait >= D("0.0001") * self.at.serv
            self.cond[name] = float(thr / s) if ok else float("inf")
            self.usable[name] = ok and self.cond[name] <= 100.0


def _case(row, kind, n, lam_exp, rate_tol, *, min_replicas=1.0, feasible=True):
    row = row.copy()
    case = {"kind": kind, "N": n, "feasible": feasible, "rate_tol": rate_tol}
    if feasible:
        rate_star = oracle.evaluate(row, lam_exp).throughput * 1000  # req/s
        row[P_TOTAL_RATE] = float((D(REPLICA_M) + D("0.5")) * rate_star)
        row[P_MIN_REPLICAS] = min_replicas
        replicas = max(REPLICA_M + 1, int(min_replicas))
        final = oracle.evaluate(row, D(float(row[P_TOTAL_RATE])) / replicas / 1000)
        case.update(rate_star=rate_star, replicas=replicas, final=final)
    else:
        row[P_TOTAL_RATE] = 10.0
        row[P_MIN_REPLICAS] = 1.0
    case["row"] = row
    return case


def cases_for_limit(n):
    """All constructed cases of one batch limit N."""
    cases = []
    shapes = SHAPES + (EXTRA_SHAPES if n in EXTRA_SHAPE_LIMITS else ())
    for si, (in_tokens, out_tokens) in enumerate(shapes):
        row = _base_row(in_tokens, out_tokens, n)
        lam_min, lam_max = oracle.rate_range(row)
        pts = {f: _Point(row, f) for f in FRACTIONS}

        def with_targets(ttft=0.0, itl=0.0, tps=0.0):
            r = row.copy()
            r[P_TARGET_TTFT], r[P_TARGET_ITL], r[P_TARGET_TPS] = float(ttft), float(itl), tps
            return r

        for f, pt in pts.items():
            for name in ("ttft", "itl"):
                if not pt.usable[name]:
                    continue  # ill-conditioned: dropped here, at construction
                r = with_targets(**{name: getattr(pt.at, name)})
                tol = 2e-6 * pt.cond[name] + 1e-9
                cases.append(_case(r, name, n, pt.lam, tol))
                if f == 0.8 and si == 0:
                    cases.append(
                        _case(r, name, n, pt.lam, tol, min_replicas=MIN_REPLICAS_ABOVE)
                    )
        for f_ttft, f_itl in BOTH_PAIRS:  # the first usable pair
            a, b = pts[f_ttft], pts[f_itl]
            if not (a.usable["ttft"] and b.usable["itl"]):
                continue
            r = with_targets(ttft=a.at.ttft, itl=b.at.itl)
            name, pt = ("ttft", a) if a.lam < b.lam else ("itl", b)
            cases.append(_case(r, "both", n, pt.lam, 2e-6 * pt.cond[name] + 1e-9))
            break

        top = oracle.evaluate(row, lam_max)
        bottom = oracle.evaluate(row, lam_min)
        cases.append(
            _case(with_targets(itl=bottom.itl / 2), "below", n, None, None, feasible=False)
        )
        # the kinds without a bisection take the same path for every
        # shape: the first shape and the single-token ones are enough,
        # and the table has to stay under 512 rows (see build_cases' end)
        if si == 0 or (in_tokens, out_tokens) in EXTRA_SHAPES:
            cases.append(
                _case(with_targets(tps=1000.0), "tps", n, lam_max * D("0.9"), FINAL_TOL)
            )
            cases.append(_case(with_targets(), "none", n, lam_max, FINAL_TOL))
            cases.append(
                _case(with_targets(ttft=2 * top.ttft, itl=2 * top.itl), "above", n, lam_max,
                      FINAL_TOL)
            )
            # a decode-only TTFT is the bare wait, which at lam_min can lie
            # under the resp - serv cancellation floor: same rule as above
            if in_tokens > 0 or bottom.wait >= D("0.0001") * bottom.serv:
                cases.append(
                    _case(with_targets(ttft=bottom.ttft / 2), "below", n, None, None,
                          feasible=False)
                )
        if si == 0:
            cases.append(
                _case(with_targets(), "none", n, lam_max, FINAL_TOL,
                      min_replicas=MIN_REPLICAS_ABOVE)
            )
        if n == 1:  # justify FLAT_ITL_CELLS from the oracle itself
            assert abs(top.itl - bottom.itl) <= D("1e-40") * top.itl
    return cases


def build_cases():
    cases = [c for n in BATCH_LIMITS for c in cases_for_limit(n)]

    # coverage: nothing the table promises may silently drop out
    have = {(c["N"], c["kind"]) for c in cases}
    for n in BATCH_LIMITS:
        for kind in KINDS:
            if (n, kind) in FLAT_ITL_CELLS:
                assert (n, kind) not in have
            else:
                assert (n, kind) in have, f"no case left for N={n}, kind={kind}"
    assert len(cases) >= 100
    # below 512 rows the launcher's auto pick is the speculative geometry
    assert len(cases) < 512
    return cases


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def problems_of(cases):
    return np.stack([c["row"] for c in cases])


def _rel(got, exact):
    return float(abs(D(float(got)) - exact) / abs(exact))


def oracle_errors(results, cases):
    """Per-case errors against the oracle plus the worst of each kind.

    A case may carry its own ``final_tol`` (test_ops_oracle_wide.py: the
    bound grows with the row's log table); without one it is FINAL_TOL."""
    assert results.shape == (len(cases), 6)
    worst = {"rate_known": 0.0, "rate_vs_bound": 0.0, "itl": 0.0, "ttft": 0.0, "rho": 0.0}
    problems = []
    for i, (res, c) in enumerate(zip(results, cases)):
        tag = f"case {i} (N={c['N']}, {c['kind']})"
        if res[R_FEASIBLE] != (1.0 if c["feasible"] else 0.0):
            problems.append(f"{tag}: feasible={res[R_FEASIBLE]}")
            continue
        if not c["feasible"]:
            if (res != 0.0).any():
                problems.append(f"{tag}: infeasible row not all-zero: {res}")
            continue
        if res[R_REPLICAS] != c["replicas"]:
            problems.append(f"{tag}: replicas={res[R_REPLICAS]}, want {c['replicas']}")
            continue
        fin = c["final"]
        errs = {
            "itl": _rel(res[R_ITL], fin.itl),
            "rho": _rel(res[R_RHO], fin.rho),
            "ttft": float(abs(D(float(res[R_TTFT])) - fin.ttft) / (fin.ttft + fin.serv)),
        }
        rate_err = _rel(res[R_RATE_STAR], c["rate_star"])
        if c["kind"] in LAM_KNOWN_KINDS:
            errs["rate_known"] = rate_err
        else:
            worst["rate_vs_bound"] = max(worst["rate_vs_bound"], rate_err / c["rate_tol"])
            if not rate_err <= c["rate_tol"]:
                problems.append(f"{tag}: rate_star err {rate_err:.3g} > {c['rate_tol']:.3g}")
        final_tol = c.get("final_tol", FINAL_TOL)
        for name, err in errs.items():
            worst[name] = max(worst[name], err)
            if "scale" in c:  # error in units of the row's float64 floor
                worst["scaled"] = max(worst.get("scaled", 0.0), err / (2.0**-53 * c["scale"]))
            if not err <= final_tol:
                problems.append(f"{tag}: {name} err {err:.3g} > {final_tol:.3g}")
    return worst, problems


def assert_matches_oracle(results, cases, label):
    assert np.isfinite(results).all(), f"{label}: non-finite output"
    infeasible = results[:, R_FEASIBLE] != 1.0
    assert (results[infeasible] == 0.0).all(), f"{label}: infeasible rows must be all-zero"
    worst, problems = oracle_errors(results, cases)
    print(f"oracle parity [{label}]: " + ", ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert not problems, f"{label}: {len(problems)} mismatches, first: " + "; ".join(problems[:5])


# rows whose replica count or per-replica rate is not positive: (total_rate,
# min_replicas).  The result must be the all-zero infeasible row.
NON_POSITIVE_LOADS = ((0.0, 0.0), (0.0, 1.0), (-1.0, 0.0))


def non_positive_problems(cases):
    rows = []
    for c in cases:
        if c["kind"] in ("none", "ttft") and c["N"] in (1, 65, 700) and c["feasible"]:
            for total_rate, min_replicas in NON_POSITIVE_LOADS:
                r = c["row"].copy()
                r[P_TOTAL_RATE], r[P_MIN_REPLICAS] = total_rate, min_replicas
                rows.append(r)
    assert len(rows) >= 3 * len(NON_POSITIVE_LOADS)
    return np.stack(rows)


def _torch_cpu(problems):
    import torch

    from wva_amd.ops import get_native

    return get_native().solve_allocations(torch.from_numpy(problems)).numpy()


def _torch_free_cpu(problems):
    from wva_amd.ops import get_native_cpu

    return get_native_cpu().solve_allocations(problems)


CPU_SOLVERS = [
    pytest.param(_solve_problems_python, id="python"),
    pytest.param(
        _torch_free_cpu,
        id="torch_free",
        marks=pytest.mark.skipif(
            not native_cpu_available(), reason="torch-free extension not built"
        ),
    ),
    pytest.param(
        _torch_cpu,
        id="torch",
        marks=pytest.mark.skipif(not native_available(), reason="native extension not built"),
    ),
]


def test_table_covers_every_kind_and_limit(cases):
    # build_cases asserts the per-cell coverage; pin the overall make-up too
    kinds = {c["kind"] for c in cases}
    assert kinds == set(KINDS)
    assert {c["N"] for c in cases} == set(BATCH_LIMITS)
    assert sum(c["feasible"] and c["replicas"] == int(MIN_REPLICAS_ABOVE) for c in cases) >= 10
    shapes = {(c["row"][4], c["row"][5]) for c in cases}
    assert shapes == {(float(i), float(o)) for i, o in SHAPES + EXTRA_SHAPES}


@pytest.mark.parametrize("solver", CPU_SOLVERS)
class TestCPUAgainstOracle:
    def test_constructed_cases(self, solver, cases):
        assert_matches_oracle(solver(problems_of(cases)), cases, "cpu")

    def test_non_positive_rate_is_infeasible(self, solver, cases):
        problems = non_positive_problems(cases)
        with warnings.catch_warnings(), np.errstate(divide="raise", invalid="raise"):
            warnings.simplefilter("error")
            out = solver(problems)
        assert np.isfinite(out).all()
        assert (out == 0.0).all()


GEOMETRIES = ["64", "128", "256", "384", "896", None]
BITWISE_GEOMETRIES = ["64", "128", "384", "896"]  # all evaluate with WgEval<64>
SAME_SCAN_LIMITS = (1, 2, 3, 4, 5)  # K = 11 * N <= 64: one state per thread everywhere


def _set_geometry(monkeypatch, threads):
    if threads is None:
        monkeypatch.delenv("WVA_GPU_THREADS", raising=False)
    else:
        monkeypatch.setenv("WVA_GPU_THREADS", threads)


def _fits_896(cases):
    # the launcher silently falls back to auto when 896 does not fit, so a
    # table with larger N would not test the 896 kernel at all
    return [c for c in cases if c["N"] <= MAX_N_896]


@pytest.mark.gpu
class TestGPUAgainstOracle:
    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_constructed_cases(self, threads, cases, monkeypatch):
        _set_geometry(monkeypatch, threads)
        table = _fits_896(cases) if threads == "896" else cases
        problems = problems_of(table)
        assert len(problems) < 512  # auto must pick the speculative geometry
        # one heterogeneous launch: N = 1 and the largest N share a max_k
        got = solve_problems(problems, device="cuda")
        assert_matches_oracle(got, table, f"gpu {threads or 'auto'}")

    def test_chip_filling_auto_launch(self, cases, monkeypatch):
        _set_geometry(monkeypatch, None)
        reps = -(-512 // len(cases))
        tiled = cases * reps
        assert len(tiled) >= 512  # auto picks the 128-thread dual geometry
        got = solve_problems(problems_of(tiled), device="cuda")
        assert_matches_oracle(got, tiled, "gpu auto B>=512")

    @pytest.mark.parametrize("threads", GEOMETRIES)
    def test_non_positive_rate_is_infeasible(self, threads, cases, monkeypatch):
        _set_geometry(monkeypatch, threads)
        problems = non_positive_problems(_fits_896(cases))
        out = solve_problems(problems, device="cuda")
        assert np.isfinite(out).all()
        assert (out == 0.0).all()

    def _solve_each(self, problems, monkeypatch):
        got = {}
        for threads in BITWISE_GEOMETRIES:
            _set_geometry(monkeypatch, threads)
            got[threads] = solve_problems(problems, device="cuda")
        return got

    def test_speculative_search_bitwise_equal_sequential(self, monkeypatch):
        """64 (sequential), 128 (dual), 384 and 896 (speculative depth 2/3)
        all evaluate with WgEval<64>, and the speculative search replays the
        sequential decision walk on the same midpoints.  With K = 11 * N <=
        64 every geometry's build_cum scans one state per thread, so the
        cumulative table — the only input that otherwise depends on the
        thread count — is summed in the same order and the outputs must be
        bit-identical; a stale or raced mailbox read would differ."""
        table = [c for n in SAME_SCAN_LIMITS for c in cases_for_limit(n)]
        assert {c["kind"] for c in table} == set(KINDS)
        got = self._solve_each(problems_of(table), monkeypatch)
        assert_matches_oracle(got["64"], table, "gpu 64, K <= 64")
        for threads in BITWISE_GEOMETRIES[1:]:
            np.testing.assert_array_equal(got[threads], got["64"], err_msg=f"{threads} vs 64")

    def test_speculative_search_same_walk_as_sequential(self, cases, monkeypatch):
        """Beyond K = 64 the chunked scan of build_cum adds log(mu) in an
        order that depends on the thread count, so the table, every y and
        the outputs differ in their last bits between geometries (measured:
        <= 2e-14 relative) and bit equality cannot hold.  What must hold is
        that all four take the same decision walk: exact feasibility and
        replicas, and rate_star — throughput at the lam the walk ended on —
        equal to within the evaluation error of the two sides, 2 *
        FINAL_TOL, for binding targets too.  A walk that differs in one
        decision ends a bracket away, orders of magnitude further."""
        table = _fits_896(cases)
        got = self._solve_each(problems_of(table), monkeypatch)
        ref = got["64"]
        for threads in BITWISE_GEOMETRIES:
            assert_matches_oracle(got[threads], table, f"gpu {threads}, N <= {MAX_N_896}")
        worst = 0.0
        for threads in BITWISE_GEOMETRIES[1:]:
            out = got[threads]
            np.testing.assert_array_equal(out[:, R_FEASIBLE], ref[:, R_FEASIBLE])
            np.testing.assert_array_equal(out[:, R_REPLICAS], ref[:, R_REPLICAS])
            feas = ref[:, R_FEASIBLE] == 1.0
            diff = np.abs(out[feas, R_RATE_STAR] / ref[feas, R_RATE_STAR] - 1.0).max()
            worst = max(worst, diff)
            print(f"rate_star {threads} vs 64: {diff:.3g}")
        assert worst <= 2 * FINAL_TOL

    def test_oversized_chain_raises_before_launch(self, cases, monkeypatch):
        """N = 716 passes a (max_k + 288)-double estimate but no kernel
        geometry an under-512-row launch may use fits its LDS: the binding
        must raise instead of returning an all-infeasible result."""
        import torch

        from wva_amd.ops import get_native

        native = get_native()
        _set_geometry(monkeypatch, None)
        row = cases[0]["row"].copy()
        row[P_MAX_BATCH] = 716.0
        with pytest.raises(RuntimeError, match="too large"):
            native.solve_allocations(torch.from_numpy(row[None, :]).cuda())
        _set_geometry(monkeypatch, "256")
        with pytest.raises(RuntimeError, match="too large"):
            native.solve_allocations(torch.from_numpy(row[None, :]).cuda())
        # the refused call left the device usable
        _set_geometry(monkeypatch, None)
        few = [c for c in cases if c["N"] in (6, 129)]
        got = native.solve_allocations(torch.from_numpy(problems_of(few)).cuda()).cpu().numpy()
        assert_matches_oracle(got, few, "gpu after refusal")
