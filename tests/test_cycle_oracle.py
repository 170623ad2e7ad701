"""The whole sizing cycle against the fleet-level oracle (tests/fleet_oracle.py).

test_ops_oracle*.py check the ``[B, 12] -> [B, 6]`` solve.  This module checks
what production runs around it: ``System`` -> rows, results -> ``Allocation``
objects (cost, transition penalty, energy term), the chunked submit/collect
pipeline, and ``Manager.optimize()`` + ``generate_solution()`` — on seeded
random fleets and on named ones (a chip-filling >= 512-row fleet, the N = 256
flagship chain, an N = 1024 server that takes the synchronous CPU split, and
exact cost ties).

Sizing stage, for every path (``System.calculate()``; the batched solver on
the pure-Python fallback, the torch-free binding and the torch CPU binding,
each in 1, 2 and 3 chunks; the gfx950 kernel in the gpu tier):

- the keys of ``all_allocations`` per server are the oracle's feasible set, in
  candidate order (the optimizer's stable sort makes the order observable);
- every Allocation, turned back into a result row, passes
  ``assert_matches_oracle``: replicas exact, ``rate_star`` within ``rate_tol``,
  final ITL/TTFT/rho within the row's ``final_tol`` — the tolerances of
  test_ops_oracle_wide.py, no new constant;
- ``accelerator``, ``batch_size``, ``cost`` and, under the cost objective,
  ``value`` are bit-equal to the expectation written from the definitions
  (cost = acc.cost * (instances * replicas)); under ``cost+energy`` the value
  is within ``final_tol * max power slope / idle power`` of the energy term;
- pairs without solver involvement (zero load) are bit-equal to the scalar
  path in every field;
- the problem matrix the batched solver hands to its dispatch equals the
  independently built rows bit for bit, in order (every solver truncates
  tokens and N itself, so a row built otherwise would not show downstream).

Optimize stage (cost-objective fleets): unlimited mode and limited mode under
every saturation policy, delayed best effort both ways, on scarce and on ample
capacity must export the scalar path's solution: accelerator, replicas and
max batch exact, cost bit-equal.  The tie fleets are the sharp cases: with
``(acc.cost * instances) * replicas`` the batched path picked the other
accelerator (values 11.55 / 11.549999999999997 where the definition ties).

Cost: the fleet table builds in about 4 s of CPU (measured and printed) and
the scalar reference of all fleets in under 1 s; every CPU case after that is
one sizing call plus a few optimizer passes (344 cases in about 11 s).
"""

from __future__ import annotations

import contextlib
import copy

import numpy as np
import pytest

import fleet_oracle as fo
import wva_amd.ops as ops
import wva_amd.ops.batched as B
from test_ops_oracle import assert_matches_oracle
from wva_amd.core import System
from wva_amd.ops import BatchedAllocationSolver, native_available, native_cpu_available
from wva_amd.solver import Manager, Optimizer

ALLOCATION_FIELDS = (
    "accelerator", "num_replicas", "batch_size", "cost", "value", "itl", "ttft",
    "rho", "max_arrv_rate_per_replica",
)
CHUNKS = (1, 2, 3)

CPU_PATHS = [
    pytest.param("python", id="python"),
    pytest.param(
        "torch_free",
        id="torch_free",
        marks=pytest.mark.skipif(
            not native_cpu_available(), reason="torch-free extension not built"
        ),
    ),
    pytest.param(
        "torch",
        id="torch",
        marks=pytest.mark.skipif(not native_available(), reason="native extension not built"),
    ),
]


@pytest.fixture(scope="module")
def fleets():
    return {f.name: f for f in fo.build_fleets()}


@contextlib.contextmanager
def sizing_env(fleet, path="scalar"):
    """The fleet's WVA_SIZING_HEADROOM and the Markovian analyzer; for a CPU
    path of the batched solver, only that implementation left loadable."""
    with pytest.MonkeyPatch.context() as mp:
        if fleet.headroom:
            mp.setenv("WVA_SIZING_HEADROOM", str(fleet.headroom))
        else:
            mp.delenv("WVA_SIZING_HEADROOM", raising=False)
        mp.delenv("WVA_ANALYZER", raising=False)
        mp.delenv("WVA_SERVICE_SCV", raising=False)
        if path == "python":
            mp.setattr(ops, "_native", None)
            mp.setattr(ops, "_native_cpu", None)
        elif path == "torch":
            mp.setattr(ops, "_native_cpu", None)  # the torch binding is second in line
        elif path == "torch_free":
            assert native_cpu_available()  # first in line as it is
        yield mp


def new_system(fleet):
    system = System()
    system.set_from_spec(fo.fresh_spec(fleet))
    return system


def sized(fleet, path, chunks=None, device="cpu"):
    """A fresh system of the fleet, sized by one path.  For the batched
    solver, ``system.submitted`` is the problem matrix it handed to its
    dispatch, all chunks in order."""
    system = new_system(fleet)
    with sizing_env(fleet, path) as mp:
        if path == "scalar":
            system.calculate()
            return system
        submitted = []
        for dispatch in (B.SyncDispatch, B.NativeGpuDispatch):
            def submit(self, problems, scv_rows=None, _real=dispatch.submit):
                submitted.append(np.array(problems, dtype=np.float64, copy=True))
                return _real(self, problems, scv_rows)

            mp.setattr(dispatch, "submit", submit)
        BatchedAllocationSolver(device=device, chunks=chunks).calculate(system)
    system.submitted = np.concatenate(submitted) if submitted else np.zeros((0, 12))
    return system


@pytest.fixture(scope="module")
def scalar(fleets):
    """``System.calculate()`` of every fleet, computed once and left alone:
    (sized system, {variant label: exported solution})."""
    out = {}
    for name, fleet in fleets.items():
        system = sized(fleet, "scalar")
        out[name] = (system, solutions_of(fleet, system))
    return out


def fields_of(alloc):
    return tuple(getattr(alloc, f) for f in ALLOCATION_FIELDS)


def check_sizing(fleet, system, scalar_system, label):
    """Every sizing-stage assertion of the module docstring, on one sized
    system.  Unconditional: a kept fleet has no ambiguous pair."""
    rows, cases = [], []
    assert list(system.servers) == [s.name for s in fleet.spec.servers.spec]
    for name, server in system.servers.items():
        pairs = fleet.pairs[name]
        allocs = server.all_allocations
        want = [p.acc for p in pairs if p.kind == "zero_load" or p.case["feasible"]]
        assert list(allocs) == want, f"{label} {name}: feasible set or its order"
        ref = scalar_system.servers[name].all_allocations
        assert list(allocs) == list(ref), f"{label} {name}: order differs from the scalar path"
        for p in pairs:
            tag = f"{label} {name}/{p.acc}"
            if p.kind == "zero_load":
                assert fields_of(allocs[p.acc]) == fields_of(ref[p.acc]), tag
                continue
            cases.append(p.case)
            if not p.case["feasible"]:
                rows.append((0.0,) * 6)
                continue
            a = allocs[p.acc]
            rows.append((1.0, a.num_replicas, a.max_arrv_rate_per_replica * 1000.0,
                         a.itl, a.ttft, a.rho))
            assert a.accelerator == p.acc, tag
            assert a.batch_size == p.batch_size, f"{tag}: N {a.batch_size}, want {p.batch_size}"
            if a.num_replicas != p.case["replicas"]:
                continue  # reported by assert_matches_oracle below, with the row
            assert a.cost == p.cost, f"{tag}: cost {a.cost!r}, want {p.cost!r}"
            if fleet.energy:
                got = a.value - p.value
                assert abs(got - p.energy) <= p.energy_tol, (
                    f"{tag}: energy part of value {got!r}, want {p.energy!r} "
                    f"+- {p.energy_tol:.3g}")
            else:
                assert a.value == p.value, f"{tag}: value {a.value!r}, want {p.value!r}"
    if hasattr(system, "submitted"):
        # the rows themselves, bit for bit: every solver truncates tokens and
        # N on its own, so only here does a row built otherwise show
        want_rows = np.stack([c["row"] for c in cases]) if cases else np.zeros((0, 12))
        assert system.submitted.shape == want_rows.shape, f"{label} {fleet.name}: row count"
        bad = np.argwhere(system.submitted != want_rows)
        assert not len(bad), (
            f"{label} {fleet.name}: row {bad[0][0]} column {bad[0][1]} is "
            f"{system.submitted[tuple(bad[0])]!r}, want {want_rows[tuple(bad[0])]!r}")
    if cases:
        assert_matches_oracle(np.array(rows, dtype=np.float64), cases, f"{label} {fleet.name}")


def solutions_of(fleet, system):
    """{variant label: {server: (accelerator, replicas, max_batch, cost)}}
    over the fleet's optimizer variants, each on a copy of the sized system."""
    if fleet.energy:
        return {}  # the optimize stage covers the cost objective
    out = {}
    for label, opt_spec, capacity in fleet.variants:
        s = copy.deepcopy(system)
        s.capacity = dict(capacity)
        s.optimizer_spec = opt_spec
        Manager(s, Optimizer(opt_spec)).optimize()
        out[label] = {
            name: (d.accelerator, d.num_replicas, d.max_batch, d.cost)
            for name, d in s.generate_solution().spec.items()
        }
    return out


def check_optimize(fleet, system, scalar_solutions, label):
    got = solutions_of(fleet, system)
    assert list(got) == list(scalar_solutions)
    for variant, want in scalar_solutions.items():
        assert list(got[variant]) == list(want), f"{label} {fleet.name} {variant}: servers"
        for name in want:
            assert got[variant][name] == want[name], (
                f"{label} {fleet.name} {variant} {name}: {got[variant][name]!r}, "
                f"scalar path {want[name]!r}")


def check_fleet(fleet, system, scalar, label):
    scalar_system, scalar_solutions = scalar[fleet.name]
    check_sizing(fleet, system, scalar_system, label)
    check_optimize(fleet, system, scalar_solutions, label)


# ---------------------------------------------------------------------------
# The table itself, and the scalar path (the semantic reference)
# ---------------------------------------------------------------------------

def test_fleet_table_covers_what_it_claims(fleets):
    # build_fleets asserted the redraw cap and the per-kind coverage
    assert tuple(fleets) == fo.FLEET_NAMES
    chip = fleets[fo.CHIP_FILLING]
    assert chip.rows() >= 512
    assert len(chip.spec.servers.spec) * len(chip.spec.accelerators.spec) >= 512
    assert max(p.batch_size for p in fleets[fo.OVERSIZED].solved_pairs()) == fo.OVERSIZED_N
    rnd = [fleets[n] for n in fo.RANDOM_NAMES]
    labels = {v[0] for f in rnd for v in f.variants}
    for policy in fo.POLICIES:
        for mode in ("grouped", "delayed"):
            assert f"scarce-{policy}-{mode}" in labels
    assert "unlimited" in labels and "ample-None-grouped" in labels
    drawn = {(f.spec.optimizer.spec.unlimited, f.spec.optimizer.spec.saturation_policy,
              f.spec.optimizer.spec.delayed_best_effort) for f in rnd}
    assert {d[0] for d in drawn} == {True, False}
    assert {d[1] for d in drawn} == set(fo.POLICIES) and {d[2] for d in drawn} == {True, False}
    servers = [s for f in rnd for s in f.spec.servers.spec]
    loads = [s.current_alloc.load for s in servers]
    assert any(ld.arrival_rate == 0 for ld in loads)
    assert any(ld.avg_in_tokens == 0 for ld in loads)
    assert any(ld.avg_in_tokens != int(ld.avg_in_tokens) for ld in loads)
    assert {0, 1} <= {ld.avg_out_tokens for ld in loads}
    assert any(ld.avg_out_tokens != int(ld.avg_out_tokens) for ld in loads)
    assert {s.min_num_replicas for s in servers} == {0, 1, 2, 3}
    assert {s.max_batch_size for s in servers} == set(fo.SERVER_MAX_BATCH)
    assert any(s.keep_accelerator for s in servers)
    for f in rnd:
        types = [a.type for a in f.spec.accelerators.spec]
        assert len(set(types)) == len(types) - 1  # two accelerators pool one type
        prios = [c.priority for c in f.spec.service_classes.spec]
        assert len(set(prios)) < len(prios)  # two classes of equal priority
    assert {a.multiplicity for f in rnd for a in f.spec.accelerators.spec} == {1, 2}


@pytest.mark.parametrize("name", fo.FLEET_NAMES)
def test_scalar_path(name, fleets, scalar):
    """``System.calculate()`` is the reference the batched path is measured
    against; it is itself held to the oracle and to the definitions."""
    system, _ = scalar[name]
    check_sizing(fleets[name], system, system, "scalar")


def test_scarce_capacity_really_binds(fleets, scalar):
    """The scarce variants must differ from the ample one somewhere, or the
    limited-mode comparisons below would all run the same grant path."""
    differing = 0
    for name in fo.RANDOM_NAMES:
        sols = scalar[name][1]
        if sols and any(sols[v] != sols["ample-None-grouped"] for v in sols if "scarce" in v):
            differing += 1
    assert differing >= 8


@pytest.mark.parametrize("name", fo.TIE_NAMES)
def test_tie_fleets_pick_the_definitions_winner(name, fleets, scalar):
    """Oracle-independent statement of the tie cases: where the definition's
    cost ties, the first accelerator in order wins; where it makes the second
    one cheaper by a last bit, the second wins."""
    want = "MI355X" if "scalar_tie" in name else "MI300X"
    for variant in ("unlimited", "ample-None-grouped"):  # greedy's stable sort too
        solution = scalar[name][1][variant]
        assert [v[0] for v in solution.values()] == [want, want], variant


# ---------------------------------------------------------------------------
# The batched solver on every CPU path
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("path", CPU_PATHS)
@pytest.mark.parametrize("name", fo.FLEET_NAMES)
def test_batched_cpu(name, path, chunks, fleets, scalar):
    fleet = fleets[name]
    system = sized(fleet, path, chunks)
    check_fleet(fleet, system, scalar, f"{path} chunks={chunks}")


@pytest.mark.parametrize("tps", [0.0, 500.0])
@pytest.mark.parametrize("path", CPU_PATHS)
def test_under_one_output_token_allocates_nothing(path, tps, fleets):
    """0 < out_tokens < 1 truncates to K = 0.  The scalar path's analyzer
    rejects that request size, so the server gets no allocation and the rest
    of the fleet is sized as usual — under a TPS target too, where the batched
    path used to divide by K before the row contract could reject the row."""
    fleet = copy.copy(fleets[fo.TIE_NAMES[0]])
    fleet.spec = fo.fresh_spec(fleet)
    fleet.spec.servers.spec[0].current_alloc.load.avg_out_tokens = 0.5
    fleet.spec.service_classes.spec[0].model_targets[0].slo_tps = tps
    first, second = (s.name for s in fleet.spec.servers.spec)
    assert fo.expected_row(fleet.spec, fleet.spec.servers.spec[0],
                           fleet.spec.accelerators.spec[0]) == ("skip", "under_one_output_token")
    ref = sized(fleet, "scalar")
    assert ref.servers[first].all_allocations == {}
    assert list(ref.servers[second].all_allocations) == ["MI355X", "MI300X"]
    for chunks in CHUNKS:
        system = sized(fleet, path, chunks)
        assert system.servers[first].all_allocations == {}
        got, want = system.servers[second].all_allocations, ref.servers[second].all_allocations
        assert list(got) == list(want)
        for acc in want:
            assert fields_of(got[acc])[:5] == fields_of(want[acc])[:5]  # through value


# ---------------------------------------------------------------------------
# The gfx950 kernel through the native submit/collect dispatch
# ---------------------------------------------------------------------------

@pytest.mark.gpu
class TestGPUCycle:
    @pytest.fixture(autouse=True)
    def _pool_is_idle_afterwards(self):
        yield
        assert ops.get_native().dispatch_pool_stats()[1] == 0

    @pytest.mark.parametrize("chunks", [1, None, 3])
    def test_small_fleets(self, chunks, fleets, scalar):
        for name in fo.RANDOM_NAMES + fo.TIE_NAMES:
            fleet = fleets[name]
            system = sized(fleet, "gpu", chunks, device="cuda")
            check_fleet(fleet, system, scalar, f"gpu chunks={chunks}")

    def test_chip_filling_fleet_is_one_launch(self, fleets, scalar):
        fleet = fleets[fo.CHIP_FILLING]
        assert fleet.rows() >= 512  # the launcher's 128-thread geometry
        system = new_system(fleet)
        dispatch, n_chunks, _ = BatchedAllocationSolver(device="cuda")._plan(
            system, list(system.servers.values()))
        assert isinstance(dispatch, B.NativeGpuDispatch) and n_chunks == 1
        system = sized(fleet, "gpu", None, device="cuda")
        check_fleet(fleet, system, scalar, "gpu >= 512 rows")

    def test_flagship_chain(self, fleets, scalar):
        fleet = fleets[fo.FLAGSHIP]
        check_fleet(fleet, sized(fleet, "gpu", None, device="cuda"), scalar, "gpu N=256")

    def test_oversized_server_takes_the_cpu_split(self, fleets, scalar, monkeypatch):
        split = []
        real = B.solve_problems

        def spy(problems, device=None):
            split.append(len(problems))
            return real(problems, device)

        # NativeGpuDispatch.submit calls solve_problems only for a chunk
        # whose largest N exceeds the LDS limit
        monkeypatch.setattr(B, "solve_problems", spy)
        fleet = fleets[fo.OVERSIZED]
        system = sized(fleet, "gpu", 2, device="cuda")
        assert split, "the synchronous split was not taken"
        check_fleet(fleet, system, scalar, "gpu N=1024, 2 chunks")

    def test_hipgraph_route(self, fleets, scalar, monkeypatch):
        monkeypatch.setattr(B, "_graph_cache", {})
        monkeypatch.setattr(B, "_graph_disabled", False)
        monkeypatch.setenv("WVA_GPU_GRAPH", "1")
        fleet = fleets[fo.RANDOM_NAMES[1]]
        for what in ("capture", "replay"):
            system = sized(fleet, "gpu", None, device="cuda")
            check_fleet(fleet, system, scalar, f"gpu graph {what}")
        assert len(B._graph_cache) == 1
        assert not B._graph_disabled  # capture really worked, no fallback
