"""The native greedy solve (csrc/greedy_core.h) against the Python greedy.

The yardstick is ``solve_greedy``'s Python body in the same tree, forced with
``WVA_NATIVE_GREEDY=0``.  Both routes run on ``copy.deepcopy``s of one
prepared system and must leave it in the same state, exactly: for every
server the chosen allocation (by its key in ``all_allocations``), all nine
fields of ``server.allocation``, ``server.spec.desired_alloc``, and the
fields of every entry of ``all_allocations`` (best effort rescales one of
them in place).  Floats are compared by their hex form, so a NaN equals a
NaN and -0.0 differs from 0.0.

A spy on the binding shows that the native route really ran on the ordinary
cases and did not on the fallback cases.
"""

from __future__ import annotations

import copy
import math
import random

import pytest

import fleet_oracle as fo
import wva_amd.solver.greedy as greedy
from wva_amd.config import (
    AcceleratorCount,
    AcceleratorSpec,
    AllocationData,
    ModelAcceleratorPerfData,
    OptimizerSpec,
    ServerLoadSpec,
    ServerSpec,
)
from wva_amd.core import Allocation, System
from wva_amd.ops import native_available, native_cpu_available
from wva_amd.solver import Manager, Optimizer

pytestmark = pytest.mark.skipif(
    not (native_available() or native_cpu_available()),
    reason="neither native extension is built",
)

ALLOCATION_FIELDS = (
    "accelerator", "num_replicas", "batch_size", "cost", "value", "itl", "ttft",
    "rho", "max_arrv_rate_per_replica",
)
DESIRED_FIELDS = ("accelerator", "num_replicas", "max_batch", "cost", "itl_average",
                  "ttft_average")
POLICIES = ("None", "PriorityExhaustive", "PriorityRoundRobin", "RoundRobin")


def exact(x):
    return x.hex() if isinstance(x, float) else x


def fields_of(alloc):
    return tuple(exact(getattr(alloc, f)) for f in ALLOCATION_FIELDS)


def state_of(system):
    """Everything a greedy solve may leave behind, per server."""
    out = {}
    for name, server in system.servers.items():
        alloc = server.allocation
        chosen = None
        if alloc is not None:
            keys = [k for k, a in server.all_allocations.items() if a is alloc]
            assert len(keys) == 1, f"{name}: the allocation is not one of the server's own"
            chosen = keys[0]
        desired = server.spec.desired_alloc
        load = desired.load
        out[name] = (
            chosen,
            None if alloc is None else fields_of(alloc),
            tuple(exact(getattr(desired, f)) for f in DESIRED_FIELDS),
            None if load is None else (exact(load.arrival_rate), exact(load.avg_in_tokens),
                                       exact(load.avg_out_tokens)),
            {k: fields_of(a) for k, a in server.all_allocations.items()},
        )
    return out


class Spy:
    """Stands in for the binding and counts the calls it passes on."""

    HAS_GREEDY = True

    def __init__(self, real):
        self.real = real
        self.calls = 0

    def greedy_solve(self, *args):
        self.calls += 1
        return self.real.greedy_solve(*args)


@pytest.fixture
def spy(monkeypatch):
    real = greedy._binding()
    assert real is not None and real.HAS_GREEDY
    s = Spy(real)
    monkeypatch.setattr(greedy, "_binding", lambda: s)
    monkeypatch.delenv("WVA_NATIVE_GREEDY", raising=False)
    return s


def solve_python(system, opt_spec, solve=greedy.solve_greedy):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("WVA_NATIVE_GREEDY", "0")
        solve(system, opt_spec)
    return system


def optimize(system, opt_spec):
    """The whole optimizer pass, as the reconciler runs it."""
    Manager(system, Optimizer(opt_spec)).optimize()


def assert_same(system, opt_spec, spy, label, native=True, solve=greedy.solve_greedy):
    """Both routes on deep copies of the prepared system; returns the native
    route's copy."""
    want = state_of(solve_python(copy.deepcopy(system), opt_spec, solve))
    before = spy.calls
    got_system = copy.deepcopy(system)
    solve(got_system, opt_spec)
    assert spy.calls - before == (1 if native else 0), (
        f"{label}: the native route {'did not run' if native else 'ran'}")
    got = state_of(got_system)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], f"{label} {name}:\n native {got[name]}\n python {want[name]}"
    return got_system


# ---------------------------------------------------------------------------
# The binding itself
# ---------------------------------------------------------------------------

def test_both_bindings_carry_the_solve():
    import wva_amd.ops as ops

    built = [m for m in (ops._native_cpu, ops._native) if m is not None]
    assert built
    for mod in built:
        assert mod.HAS_GREEDY is True and callable(mod.greedy_solve)


def test_switch_is_read_per_call(spy, monkeypatch):
    system = hand_built(random.Random(5), 0)
    opt = OptimizerSpec(unlimited=False, saturation_policy="RoundRobin")
    greedy.solve_greedy(copy.deepcopy(system), opt)
    assert spy.calls == 1
    monkeypatch.setenv("WVA_NATIVE_GREEDY", "0")
    greedy.solve_greedy(copy.deepcopy(system), opt)
    assert spy.calls == 1
    monkeypatch.setenv("WVA_NATIVE_GREEDY", "1")
    greedy.solve_greedy(copy.deepcopy(system), opt)
    assert spy.calls == 2


def test_no_binding_takes_the_python_body(monkeypatch):
    monkeypatch.setattr(greedy, "_binding", lambda: None)
    monkeypatch.delenv("WVA_NATIVE_GREEDY", raising=False)
    system = hand_built(random.Random(6), 0)
    opt = OptimizerSpec(unlimited=False, saturation_policy="PriorityExhaustive")
    got = copy.deepcopy(system)
    greedy.solve_greedy(got, opt)
    assert state_of(got) == state_of(solve_python(copy.deepcopy(system), opt))


# ---------------------------------------------------------------------------
# Fleet table
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sized_fleets():
    """Every fleet under the cost objective, scalar-sized once and left
    alone: {name: (fleet, sized system)}."""
    out = {}
    for fleet in fo.build_fleets():
        if fleet.energy:
            continue
        with pytest.MonkeyPatch.context() as mp:
            if fleet.headroom:
                mp.setenv("WVA_SIZING_HEADROOM", str(fleet.headroom))
            else:
                mp.delenv("WVA_SIZING_HEADROOM", raising=False)
            mp.delenv("WVA_ANALYZER", raising=False)
            mp.delenv("WVA_SERVICE_SCV", raising=False)
            system = System()
            system.set_from_spec(fo.fresh_spec(fleet))
            system.calculate()
        out[fleet.name] = (fleet, system)
    return out


COST_FLEETS = tuple(
    name for i, name in enumerate(fo.FLEET_NAMES)
    if not (i < len(fo.RANDOM_SEEDS) and i % 4 == 3)  # random_fleet: the energy fleets
)


def test_fleet_names_are_the_cost_fleets(sized_fleets):
    assert tuple(sized_fleets) == COST_FLEETS
    assert set(fo.TIE_NAMES) <= set(sized_fleets)


@pytest.mark.parametrize("name", COST_FLEETS)
def test_fleet_table(name, sized_fleets, spy):
    fleet, system = sized_fleets[name]
    limited = 0
    for label, opt_spec, capacity in fleet.variants:
        limited += not opt_spec.unlimited
        prepared = copy.deepcopy(system)
        prepared.capacity = dict(capacity)
        prepared.optimizer_spec = opt_spec
        # the unlimited variants take the argmin solve, and a model the fleet
        # does not know is a fallback condition
        native = not opt_spec.unlimited and all(
            s.model_name in prepared.models
            for s in prepared.servers.values() if s.all_allocations)
        assert_same(prepared, opt_spec, spy, f"{name} {label}", native=native, solve=optimize)
    assert limited >= 1


# ---------------------------------------------------------------------------
# Seeded hand-built systems: no sizing, all_allocations set directly
# ---------------------------------------------------------------------------

ACCS = (("A", "T0"), ("B", "T1"), ("C", "T1"), ("D", "T2"))  # B and C share a pool
MODELS = ("m0", "m1")
CLASSES = (("gold", 1), ("silver", 2), ("bronze", 3))
POWERS_OF_TWO = (1, 2, 4, 8)
VALUES = (0.0, 1.0, 2.0, 3.0, 5.0)  # few, so that ties are common
REPLICAS = (0, 1, 1, 2, 3, 4, 6)
CAPACITIES = (0, 0, 1, 2, 4, 8, 12, 16, 32, 64)
N_SYSTEMS = 2000


def hand_built(rng, index):
    """A small system with candidates but no sizing behind them."""
    system = System()
    for name, type_name in ACCS:
        system.add_accelerator(AcceleratorSpec(name=name, type=type_name, cost=1.0,
                                               multiplicity=rng.choice(POWERS_OF_TWO)))
    for m in MODELS:
        for name, _ in ACCS:
            system.add_model_perf_data(ModelAcceleratorPerfData(
                name=m, acc=name, acc_count=rng.choice(POWERS_OF_TWO)))
    for name, prio in CLASSES:
        system.add_service_class(name, prio)
    types = ["T0", "T1", "T2"]
    if index % 3 == 0:
        types.remove(rng.choice(types))  # a type the capacity does not name
    for t in types:
        system.set_capacity(AcceleratorCount(type=t, count=rng.choice(CAPACITIES)))
    for i in range(rng.randint(1, 12)):
        spec = ServerSpec(
            name=f"s{i}", class_name=rng.choice(CLASSES)[0], model=rng.choice(MODELS),
            current_alloc=AllocationData(load=ServerLoadSpec(arrival_rate=60.0)))
        system.add_server(spec)
        server = system.servers[spec.name]
        for name, _ in rng.sample(ACCS, rng.randint(1, 4)):
            replicas = rng.choice(REPLICAS)
            alloc = Allocation(accelerator=name, num_replicas=replicas, batch_size=8,
                               cost=1.5 * replicas, itl=3.0, ttft=30.0, rho=0.5,
                               max_arrv_rate_per_replica=0.01)
            alloc.set_value(rng.choice(VALUES))
            if rng.random() < 0.03:
                alloc.accelerator = ""  # the empty zero-load allocation's
            server.all_allocations[name] = alloc
    return system


def units_of(system, server, alloc):
    acc = system.accelerator(alloc.accelerator)
    return system.model(server.model_name).get_num_instances(alloc.accelerator) * acc.multiplicity


def input_features(system):
    """What the inputs alone guarantee about the solve.

    - "miss": a server with several candidates whose cheapest one asks for
      more units than its type's whole capacity: it misses whenever it comes
      to the front, and is reinserted with its next candidate.
    - "runs off": every candidate of a server asks for more than its type's
      whole capacity, so the entry runs off its last one.
    - "tie": two servers of one priority start with equal deltas and equal
      current values, so their sort keys are equal.
    """
    found = set()
    keys = {}
    for server in system.servers.values():
        allocs = sorted(server.all_allocations.values(), key=lambda a: a.value)
        over = [
            system.accelerator(a.accelerator) is not None
            and a.num_replicas * units_of(system, server, a)
            > system.capacity.get(system.accelerator(a.accelerator).type, 0)
            for a in allocs
        ]  # False for an unknown accelerator: that entry vanishes instead
        if len(allocs) > 1 and over[0]:
            found.add("miss")
        if all(over):
            found.add("runs off")
        delta = allocs[1].value - allocs[0].value if len(allocs) > 1 else math.inf
        key = (server.priority(system), delta, allocs[0].value)
        if key in keys:
            found.add("tie")
        keys[key] = server.name
    return found


def restore(system, snapshot):
    """Put a hand-built system back into its prepared state: fresh
    allocation objects, no chosen allocation, an empty desired allocation."""
    for server, candidates in zip(system.servers.values(), snapshot):
        server.allocation = None
        server.spec.desired_alloc = AllocationData()
        server.all_allocations = {}
        for key, fields in candidates:
            alloc = Allocation()
            for f, v in zip(ALLOCATION_FIELDS, fields):
                setattr(alloc, f, v)
            server.all_allocations[key] = alloc


def test_seeded_hand_built_systems(spy):
    """All four policies, best effort delayed or not, on N_SYSTEMS systems.
    The first 40 systems go through assert_same (deep copies); the others
    are put back into the prepared state between solves, which is the same
    thing for a system that holds nothing but its candidates."""
    rng = random.Random(20260)
    features = set()
    solves = 0
    for index in range(N_SYSTEMS):
        system = hand_built(rng, index)
        features |= input_features(system)
        snapshot = [
            [(k, tuple(getattr(a, f) for f in ALLOCATION_FIELDS))
             for k, a in server.all_allocations.items()]
            for server in system.servers.values()
        ]
        for policy in POLICIES:
            for delayed in (False, True):
                opt = OptimizerSpec(unlimited=False, saturation_policy=policy,
                                    delayed_best_effort=delayed)
                label = f"system {index} {policy} delayed={delayed}"
                solves += 1
                if index < 40:
                    assert_same(system, opt, spy, label)
                    continue
                restore(system, snapshot)
                want = state_of(solve_python(system, opt))
                restore(system, snapshot)
                before = spy.calls
                greedy.solve_greedy(system, opt)
                assert spy.calls == before + 1, f"{label}: the native route did not run"
                assert state_of(system) == want, label
    assert features == {"miss", "runs off", "tie"}, features
    assert spy.calls == solves


# ---------------------------------------------------------------------------
# Named edges
# ---------------------------------------------------------------------------

def edge_system(candidates, capacity=(("T0", 8), ("T1", 8)), model="m0"):
    """candidates: per server a list of (accelerator, replicas, value)."""
    system = System()
    system.add_accelerator(AcceleratorSpec(name="A", type="T0", cost=1.0))
    system.add_accelerator(AcceleratorSpec(name="B", type="T1", cost=1.0, multiplicity=2))
    for acc in ("A", "B"):
        system.add_model_perf_data(ModelAcceleratorPerfData(name="m0", acc=acc, acc_count=1))
    system.add_service_class("gold", 1)
    for t, c in capacity:
        system.set_capacity(AcceleratorCount(type=t, count=c))
    for i, allocs in enumerate(candidates):
        spec = ServerSpec(name=f"e{i}", class_name="gold", model=model,
                          current_alloc=AllocationData(load=ServerLoadSpec(arrival_rate=60.0)))
        system.add_server(spec)
        for j, (acc, replicas, value) in enumerate(allocs):
            alloc = Allocation(accelerator=acc, num_replicas=replicas, batch_size=4,
                               cost=2.0 * replicas)
            alloc.set_value(value)
            system.servers[spec.name].all_allocations[acc or f"empty{j}"] = alloc
    return system


ALL_CONFIGS = [(p, d) for p in POLICIES for d in (False, True)]


@pytest.mark.parametrize("policy,delayed", ALL_CONFIGS)
class TestNamedEdges:
    def check(self, system, policy, delayed, spy, native=True):
        opt = OptimizerSpec(unlimited=False, saturation_policy=policy, delayed_best_effort=delayed)
        return assert_same(system, opt, spy, f"{policy} delayed={delayed}", native=native)

    def test_no_servers(self, policy, delayed, spy):
        self.check(edge_system([]), policy, delayed, spy)

    def test_server_without_allocations(self, policy, delayed, spy):
        solved = self.check(edge_system([[], [("A", 2, 1.0)]]), policy, delayed, spy)
        assert solved.servers["e0"].allocation is None
        assert solved.servers["e1"].allocation is not None

    def test_single_allocation_has_an_infinite_delta(self, policy, delayed, spy):
        # e1's only candidate (delta inf) goes before e0's pair (delta 1)
        # and takes the pool e0's cheaper candidate needs
        system = edge_system([[("A", 6, 1.0), ("B", 1, 2.0)], [("A", 4, 9.0)]])
        solved = self.check(system, policy, delayed, spy)
        assert solved.servers["e1"].allocation.accelerator == "A"
        assert solved.servers["e0"].allocation.accelerator == "B"

    @pytest.mark.parametrize("unknown", ["", "no-such-accelerator"])
    def test_unknown_accelerator_vanishes(self, unknown, policy, delayed, spy):
        # e0 misses on A, comes to the unknown candidate and is dropped: not
        # even best effort gives it the 3 units of A that are left
        system = edge_system([[("A", 9, 1.0), (unknown, 0, 2.0)], [("A", 5, 1.0)]])
        solved = self.check(system, policy, delayed, spy)
        assert solved.servers["e0"].allocation is None
        assert solved.servers["e1"].allocation is not None

    def test_zero_replicas_on_a_real_accelerator(self, policy, delayed, spy):
        system = edge_system([[("A", 0, 0.0)], [("A", 9, 1.0), ("B", 0, 4.0)]],
                             capacity=(("T0", 0),))
        solved = self.check(system, policy, delayed, spy)
        assert solved.servers["e0"].allocation.num_replicas == 0
        assert solved.servers["e1"].allocation.accelerator == "B"

    def test_partial_grant_is_rescaled_alike(self, policy, delayed, spy):
        system = edge_system([[("A", 7, 2.1), ("B", 9, 2.7)], [("A", 5, 0.3)]],
                             capacity=(("T0", 6), ("T1", 5)))
        self.check(system, policy, delayed, spy)

    @pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
    def test_non_finite_value_falls_back(self, bad, policy, delayed, spy):
        system = edge_system([[("A", 2, bad), ("B", 1, 1.0)], [("A", 7, 1.0), ("B", 3, bad)]])
        self.check(system, policy, delayed, spy, native=False)

    def test_huge_replica_count_falls_back(self, policy, delayed, spy):
        huge = 2 ** 62 - 1
        system = edge_system([[("B", huge, 1.0), ("A", 3, 2.0)], [("A", huge, 1.0)]])
        self.check(system, policy, delayed, spy, native=False)

    def test_integer_beyond_int64_falls_back(self, policy, delayed, spy):
        system = edge_system([[("A", 2 ** 70, 1.0), ("B", 2, 2.0)]],
                             capacity=(("T0", 2 ** 80), ("T1", 1)))
        self.check(system, policy, delayed, spy, native=False)

    def test_missing_model_falls_back(self, policy, delayed, spy):
        system = edge_system([[("A", 2, 1.0)]], model="no-such-model")
        solved = self.check(system, policy, delayed, spy, native=False)
        assert solved.servers["e0"].allocation is None


# ---------------------------------------------------------------------------
# One flagship-shaped cycle on the GPU
# ---------------------------------------------------------------------------

def flagship_spec(n_variants=64):
    """64 variants x 3 accelerator types at N = 256 under the benchmark's
    capacity rule: whole 8-GPU MI355X nodes for (38 n + 7) // 8 * 8 cards,
    8 n cards of each of the two other types; PriorityRoundRobin."""
    from wva_amd.config import (
        AcceleratorData, CapacityData, DecodeParmsSpec, ModelData, ModelTarget,
        OptimizerData, PrefillParmsSpec, ServerData, ServiceClassData, ServiceClassSpec,
        SystemSpec,
    )
    from wva_amd.config.mi355x import MI355X_CATALOG

    rng = random.Random(355)
    models = {"llama-8b": (1.0, 1), "llama-70b": (3.0, 4), "mixtral-8x7b": (2.0, 2)}
    slow = {"MI355X": 1.0, "MI300X": 1.6, "L40S": 6.0}
    classes = (("Premium", 1, 1.0), ("Freemium", 10, 3.0))
    perf = [
        ModelAcceleratorPerfData(
            name=m, acc=a, acc_count=count, max_batch_size=256,
            decode_parms=DecodeParmsSpec(alpha=3.0 * scale * slow[a], beta=0.03 * scale * slow[a]),
            prefill_parms=PrefillParmsSpec(gamma=8.0 * scale * slow[a],
                                           delta=0.0004 * scale * slow[a]))
        for m, (scale, count) in models.items() for a in MI355X_CATALOG
    ]
    servers = []
    for i in range(n_variants):
        model = list(models)[i % 3]
        servers.append(ServerSpec(
            name=f"va-{i}:flagship", class_name=classes[(i // 3) % 2][0], model=model,
            min_num_replicas=1, max_batch_size=256,
            current_alloc=AllocationData(
                accelerator="MI355X", num_replicas=rng.randint(1, 7),
                load=ServerLoadSpec(arrival_rate=rng.uniform(30.0, 36000.0),
                                    avg_in_tokens=rng.randint(64, 2047),
                                    avg_out_tokens=rng.randint(32, 1023)))))
    nodes = max(1, (n_variants * 38 + 7) // 8)
    return SystemSpec(
        accelerators=AcceleratorData(spec=list(MI355X_CATALOG.values())),
        models=ModelData(perf_data=perf),
        service_classes=ServiceClassData(spec=[
            ServiceClassSpec(name=name, priority=prio, model_targets=[
                ModelTarget(model=m, slo_itl=20.0 * scale * loose, slo_ttft=800.0 * scale * loose)
                for m, (scale, _) in models.items()])
            for name, prio, loose in classes]),
        servers=ServerData(spec=servers),
        optimizer=OptimizerData(spec=OptimizerSpec(unlimited=False,
                                                   saturation_policy="PriorityRoundRobin")),
        capacity=CapacityData(count=[
            AcceleratorCount(type="AMD-MI355X-288GB", count=8 * nodes),
            AcceleratorCount(type="AMD-MI300X-192GB", count=8 * n_variants),
            AcceleratorCount(type="EMU-L40S-48GB", count=8 * n_variants)]),
    )


@pytest.mark.gpu
def test_flagship_cycle_on_the_gpu(spy):
    from wva_amd.ops import BatchedAllocationSolver

    system = System()
    opt_spec = system.set_from_spec(flagship_spec())
    BatchedAllocationSolver(device="cuda").calculate(system)
    assert sum(len(s.all_allocations) for s in system.servers.values()) > 64

    exported = {}
    for route in ("python", "native"):
        s = copy.deepcopy(system)
        with pytest.MonkeyPatch.context() as mp:
            if route == "python":
                mp.setenv("WVA_NATIVE_GREEDY", "0")
            Manager(s, Optimizer(opt_spec)).optimize()
        exported[route] = (
            {name: tuple(exact(getattr(d, f)) for f in DESIRED_FIELDS)
             for name, d in s.generate_solution().spec.items()},
            state_of(s),
        )
    assert spy.calls == 1
    assert exported["native"][0], "nothing was allocated"
    assert exported["native"] == exported["python"]
