"""The greedy solve with its inputs read inside the binding
(csrc/greedy_py.h: greedy_solve_objects) against the array route and the
Python body.

Three routes leave one prepared system in three deep copies (or in one
system put back between solves):

- "objects": ``solve_greedy`` as it runs by default;
- "arrays": the binding without ``HAS_GREEDY_OBJECTS``, so that ``_marshal``
  and ``greedy_solve`` run as they did before the binding read objects;
- "python": ``WVA_NATIVE_GREEDY=0``.

They must agree field for field and bit for bit on what
``test_greedy_native.state_of`` collects: the chosen allocation by identity,
its nine fields, ``spec.desired_alloc``, and every candidate's fields.  A
recorder around the binding shows which entry points ran and whether the
object entry point solved or handed the system on (returned None).

The helpers and the seeded generator are those of tests/test_greedy_native.py.
"""

from __future__ import annotations

import copy
import faulthandler
import math
import random

import numpy as np
import pytest

import test_greedy_native as base
import wva_amd.solver.greedy as greedy
from wva_amd.config import AcceleratorSpec, OptimizerSpec
from wva_amd.core import Allocation
from wva_amd.ops import native_available, native_cpu_available
from wva_amd.solver import Manager, Optimizer

pytestmark = pytest.mark.skipif(
    not (native_available() or native_cpu_available()),
    reason="neither native extension is built",
)

state_of, solve_python = base.state_of, base.solve_python
ALL_CONFIGS = base.ALL_CONFIGS


class Recorder:
    """Stands in for the binding, passes every call on and counts them."""

    HAS_GREEDY = True
    HAS_GREEDY_OBJECTS = True

    def __init__(self, real):
        self.real = real
        self.array_calls = self.object_calls = self.object_solved = 0

    def greedy_solve(self, *args):
        self.array_calls += 1
        return self.real.greedy_solve(*args)

    def greedy_solve_objects(self, *args):
        self.object_calls += 1
        out = self.real.greedy_solve_objects(*args)
        self.object_solved += out is not None
        return out

    def counts(self):
        return self.object_calls, self.object_solved, self.array_calls


OBJECTS = (1, 1, 0)  # the object entry point solved
ARRAYS = (1, 0, 1)  # it handed on, and _marshal took the array route
PYTHON = (1, 0, 0)  # it handed on, and so did _marshal


_find_binding = greedy._binding  # as imported: tests patch the attribute, not this


def real_binding():
    real = _find_binding()
    assert real is not None and real.HAS_GREEDY_OBJECTS
    return real


@pytest.fixture
def recorder(monkeypatch):
    r = Recorder(real_binding())
    monkeypatch.setattr(greedy, "_binding", lambda: r)
    monkeypatch.delenv("WVA_NATIVE_GREEDY", raising=False)
    return r


def solve_arrays(system, opt_spec, solve=greedy.solve_greedy):
    """The route of a binding that does not read objects."""
    with pytest.MonkeyPatch.context() as mp:
        spy = base.Spy(real_binding())
        mp.setattr(greedy, "_binding", lambda: spy)
        mp.delenv("WVA_NATIVE_GREEDY", raising=False)
        solve(system, opt_spec)
    return system, spy.calls


def make_stale(system):
    """Give every server an allocation that is none of its candidates: a
    route that forgets to clear a server shows in state_of."""
    for server in system.servers.values():
        server.allocation = Allocation(accelerator="stale", num_replicas=99)


def assert_three_routes(system, opt_spec, recorder, label, expect, arrays_native=True,
                        solve=greedy.solve_greedy):
    """All three routes on deep copies of the prepared system; ``expect`` is
    what the recorder must count for the default route.  Returns that route's
    copy."""
    make_stale(system)
    want = state_of(solve_python(copy.deepcopy(system), opt_spec, solve))
    via_arrays, array_calls = solve_arrays(copy.deepcopy(system), opt_spec, solve)
    assert array_calls == (1 if arrays_native else 0), label
    assert state_of(via_arrays) == want, f"{label}: arrays against python"
    before = recorder.counts()
    got_system = copy.deepcopy(system)
    solve(got_system, opt_spec)
    ran = tuple(a - b for a, b in zip(recorder.counts(), before))
    assert ran == expect, f"{label}: (object calls, solved there, array calls) = {ran}"
    got = state_of(got_system)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], f"{label} {name}:\n objects {got[name]}\n python  {want[name]}"
    return got_system


def test_both_bindings_carry_the_entry_point():
    import wva_amd.ops as ops

    built = [m for m in (ops._native_cpu, ops._native) if m is not None]
    assert built
    for mod in built:
        assert mod.HAS_GREEDY_OBJECTS is True and callable(mod.greedy_solve_objects)
        assert mod.HAS_GREEDY is True and callable(mod.greedy_solve)


def test_switch_still_selects_the_python_body(recorder, monkeypatch):
    system = base.hand_built(random.Random(5), 0)
    opt = OptimizerSpec(unlimited=False, saturation_policy="RoundRobin")
    greedy.solve_greedy(copy.deepcopy(system), opt)
    assert recorder.counts() == OBJECTS
    monkeypatch.setenv("WVA_NATIVE_GREEDY", "0")
    greedy.solve_greedy(copy.deepcopy(system), opt)
    assert recorder.counts() == OBJECTS


# ---------------------------------------------------------------------------
# Seeded hand-built systems
# ---------------------------------------------------------------------------

N_SYSTEMS = 600


def hand_built_with_gaps(rng, index):
    """base.hand_built, with some servers left without candidates."""
    system = base.hand_built(rng, index)
    for server in system.servers.values():
        if rng.random() < 0.15:
            server.all_allocations = {}
    return system


def test_seeded_systems_on_three_routes(recorder, monkeypatch):
    """All four policies, best effort delayed or not.  The first 24 systems
    go through deep copies; the others are put back into the prepared state
    between solves (they hold nothing but their candidates)."""
    marshals = []
    real_marshal = greedy._marshal
    monkeypatch.setattr(greedy, "_marshal", lambda s: marshals.append(1) or real_marshal(s))
    rng = random.Random(20261)
    features = set()
    solves = 0
    for index in range(N_SYSTEMS):
        system = hand_built_with_gaps(rng, index)
        features |= base.input_features(_View(system))
        if any(not s.all_allocations for s in system.servers.values()):
            features.add("empty")
        snapshot = [
            [(k, tuple(getattr(a, f) for f in base.ALLOCATION_FIELDS))
             for k, a in server.all_allocations.items()]
            for server in system.servers.values()
        ]
        asked = {s.name: {k: a.num_replicas for k, a in s.all_allocations.items()}
                 for s in system.servers.values()}
        for policy, delayed in ALL_CONFIGS:
            opt = OptimizerSpec(unlimited=False, saturation_policy=policy,
                                delayed_best_effort=delayed)
            label = f"system {index} {policy} delayed={delayed}"
            solves += 1
            if index < 24:
                marshalled = len(marshals)
                assert_three_routes(system, opt, recorder, label, OBJECTS)
                assert len(marshals) == marshalled + 1, "only the array route marshals"
                continue
            base.restore(system, snapshot)
            make_stale(system)
            want = state_of(solve_python(system, opt))
            base.restore(system, snapshot)
            make_stale(system)
            via_arrays, array_calls = solve_arrays(system, opt)
            assert array_calls == 1 and state_of(via_arrays) == want, f"{label}: arrays"
            base.restore(system, snapshot)
            make_stale(system)
            before, marshalled = recorder.counts(), len(marshals)
            greedy.solve_greedy(system, opt)
            ran = tuple(a - b for a, b in zip(recorder.counts(), before))
            assert ran == OBJECTS and len(marshals) == marshalled, f"{label}: {ran}"
            assert state_of(system) == want, label
            for server in system.servers.values():
                a = server.allocation
                if a is not None and a.num_replicas != asked[server.name][_key_of(server, a)]:
                    features.add("partial grant")
    assert features == {"miss", "runs off", "tie", "empty", "partial grant"}, features
    assert recorder.object_solved == solves and recorder.array_calls == 0


def _key_of(server, alloc):
    return next(k for k, a in server.all_allocations.items() if a is alloc)


class _View:
    """A system's servers that have candidates, for base.input_features."""

    def __init__(self, system):
        self._system = system
        self.servers = {n: s for n, s in system.servers.items() if s.all_allocations}
        self.capacity = system.capacity

    def __getattr__(self, name):
        return getattr(self._system, name)


# ---------------------------------------------------------------------------
# One case per rule
# ---------------------------------------------------------------------------

def set_field(system, server, key, field, value):
    setattr(system.servers[server].all_allocations[key], field, value)


@pytest.mark.parametrize("policy,delayed", ALL_CONFIGS)
class TestRules:
    def check(self, system, policy, delayed, recorder, expect, arrays_native=True):
        opt = OptimizerSpec(unlimited=False, saturation_policy=policy, delayed_best_effort=delayed)
        return assert_three_routes(system, opt, recorder, f"{policy} delayed={delayed}", expect,
                                   arrays_native=arrays_native)

    # -- solved by the object entry point ----------------------------------
    def test_zero_servers(self, policy, delayed, recorder):
        self.check(base.edge_system([]), policy, delayed, recorder, OBJECTS)

    def test_servers_without_candidates(self, policy, delayed, recorder):
        solved = self.check(base.edge_system([[], [("A", 2, 1.0)], []]), policy, delayed,
                            recorder, OBJECTS)
        assert solved.servers["e0"].allocation is None
        assert solved.servers["e1"].allocation is not None
        assert solved.servers["e2"].allocation is None

    @pytest.mark.parametrize("unknown", ["", "no-such-accelerator"])
    def test_accelerator_missing_from_the_system(self, unknown, policy, delayed, recorder):
        # type -1, units 0: e0 misses on A, comes to the unknown candidate
        # and vanishes; best effort gives it nothing either
        system = base.edge_system([[("A", 9, 1.0), (unknown, 0, 2.0)], [("A", 5, 1.0)]])
        solved = self.check(system, policy, delayed, recorder, OBJECTS)
        assert solved.servers["e0"].allocation is None
        assert solved.servers["e1"].allocation is not None

    def test_pair_the_model_has_no_count_for(self, policy, delayed, recorder):
        # accelerator C is in the system, the model has no row for it: 0 units
        system = base.edge_system([[("A", 9, 1.0), ("C", 3, 2.0)], [("A", 5, 1.0)]])
        system.add_accelerator(AcceleratorSpec(name="C", type="T1", cost=1.0))
        self.check(system, policy, delayed, recorder, OBJECTS)

    def test_partial_grant(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 7, 2.1), ("B", 9, 2.7)], [("A", 5, 0.3)]],
                                  capacity=(("T0", 6), ("T1", 5)))
        self.check(system, policy, delayed, recorder, OBJECTS)

    def test_integer_value(self, policy, delayed, recorder):
        # an exact int is read as array('d') converts it
        system = base.edge_system([[("A", 7, 3), ("B", 2, 1)], [("A", 5, 2)]])
        self.check(system, policy, delayed, recorder, OBJECTS)

    @pytest.mark.parametrize("replicas", [2 ** 31 - 1, -(2 ** 31) + 1])
    def test_replicas_just_inside_the_bound(self, replicas, policy, delayed, recorder):
        system = base.edge_system([[("A", replicas, 1.0), ("B", 2, 2.0)], [("A", 3, 1.0)]])
        self.check(system, policy, delayed, recorder, OBJECTS)

    def test_units_just_inside_the_bound(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 1, 1.0), ("B", 2, 2.0)]], capacity=(("T0", 5000),))
        system.accelerators["A"].spec.multiplicity = 2 ** 12 - 1
        self.check(system, policy, delayed, recorder, OBJECTS)

    # -- handed on, and ending in the Python body --------------------------
    def test_missing_model(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 2, 1.0)]], model="no-such-model")
        solved = self.check(system, policy, delayed, recorder, PYTHON, arrays_native=False)
        assert solved.servers["e0"].allocation is None

    @pytest.mark.parametrize("bad", [math.nan, math.inf])
    def test_non_finite_value(self, bad, policy, delayed, recorder):
        system = base.edge_system([[("A", 2, bad), ("B", 1, 1.0)], [("A", 7, 1.0), ("B", 3, bad)]])
        self.check(system, policy, delayed, recorder, PYTHON, arrays_native=False)

    def test_overflowing_sum(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 2, 1e308), ("B", 1, 1.7e308)], [("A", 7, 1.0)]])
        self.check(system, policy, delayed, recorder, PYTHON, arrays_native=False)

    @pytest.mark.parametrize("replicas", [2 ** 31, -(2 ** 31)])
    def test_replicas_at_the_bound(self, replicas, policy, delayed, recorder):
        system = base.edge_system([[("A", replicas, 1.0), ("B", 2, 2.0)], [("A", 3, 1.0)]])
        self.check(system, policy, delayed, recorder, PYTHON, arrays_native=False)

    def test_units_at_the_bound(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 1, 1.0), ("B", 2, 2.0)]], capacity=(("T0", 5000),))
        system.accelerators["A"].spec.multiplicity = 2 ** 12
        self.check(system, policy, delayed, recorder, PYTHON, arrays_native=False)

    def test_integer_beyond_int64(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 2 ** 70, 1.0), ("B", 2, 2.0)]],
                                  capacity=(("T0", 2 ** 80), ("T1", 1)))
        self.check(system, policy, delayed, recorder, (0, 0, 0), arrays_native=False)

    # -- handed on, and solved by the array route --------------------------
    def test_huge_but_finite_values_are_left_to_marshal(self, policy, delayed, recorder):
        # beyond the object entry point's own magnitude bound, finite in sum
        system = base.edge_system([[("A", 2, 1e305), ("B", 1, -1e305)], [("A", 7, 1.0)]])
        self.check(system, policy, delayed, recorder, ARRAYS)

    def test_allocation_subclass(self, policy, delayed, recorder):
        class Tagged(Allocation):
            __slots__ = ()

        system = base.edge_system([[("A", 7, 2.0), ("B", 2, 1.0)], [("A", 5, 2.0)]])
        old = system.servers["e0"].all_allocations["B"]
        new = Tagged(accelerator="B", num_replicas=old.num_replicas, batch_size=old.batch_size,
                     cost=old.cost)
        new.set_value(old.value)
        system.servers["e0"].all_allocations["B"] = new
        self.check(system, policy, delayed, recorder, ARRAYS)

    def test_numpy_scalar_value(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 7, 2.1), ("B", 9, 2.7)], [("A", 5, 0.3)]],
                                  capacity=(("T0", 6), ("T1", 5)))
        set_field(system, "e0", "A", "value", np.float64(2.1))
        self.check(system, policy, delayed, recorder, ARRAYS)

    def test_numpy_scalar_replicas(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 7, 2.1), ("B", 9, 2.7)], [("A", 5, 0.3)]],
                                  capacity=(("T0", 6), ("T1", 5)))
        set_field(system, "e1", "A", "num_replicas", np.int64(5))
        self.check(system, policy, delayed, recorder, ARRAYS)

    def test_bool_replicas(self, policy, delayed, recorder):
        system = base.edge_system([[("A", True, 2.0), ("B", 2, 1.0)], [("A", 5, 2.0)]])
        self.check(system, policy, delayed, recorder, ARRAYS)

    def test_bool_value(self, policy, delayed, recorder):
        system = base.edge_system([[("A", 1, True), ("B", 2, 3.0)], [("A", 5, 2.0)]])
        self.check(system, policy, delayed, recorder, ARRAYS)


def test_a_subclassed_server_still_has_its_methods_called(recorder):
    """set_allocation and remove_allocation stay method calls."""
    from wva_amd.core import Server

    calls = []

    class Watched(Server):
        def set_allocation(self, alloc):
            calls.append(("set", self.name))
            super().set_allocation(alloc)

        def remove_allocation(self):
            calls.append(("remove", self.name))
            super().remove_allocation()

    system = base.edge_system([[("A", 2, 1.0)], [("A", 99, 1.0)]])
    for server in system.servers.values():
        server.__class__ = Watched
    opt = OptimizerSpec(unlimited=False, saturation_policy="None")
    greedy.solve_greedy(system, opt)
    assert recorder.counts() == OBJECTS
    assert calls == [("remove", "e0"), ("remove", "e1"), ("set", "e0")]
    assert system.servers["e1"].allocation is None


# ---------------------------------------------------------------------------
# One small flagship-profile cycle on the GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_small_flagship_cycle_on_the_gpu(recorder):
    """6 servers x 3 accelerators at N = 256 with the benchmark's profiles,
    sized on the GPU in 2 chunks, then solved on the three routes."""
    import bench
    from wva_amd.core import System
    from wva_amd.ops import BatchedAllocationSolver

    faulthandler.dump_traceback_later(120, exit=True)  # this case's own time limit
    try:
        system = System()
        opt_spec = system.set_from_spec(bench.build_system_spec(0, 0, 6))
        BatchedAllocationSolver(device="cuda", chunks=2).calculate(system)
        assert sum(len(s.all_allocations) for s in system.servers.values()) > 6

        def exported(s):
            return (
                {name: tuple(base.exact(getattr(d, f)) for f in base.DESIRED_FIELDS)
                 for name, d in s.generate_solution().spec.items()},
                state_of(s),
            )

        def optimize(s, spec):
            Manager(s, Optimizer(spec)).optimize()

        on = copy.deepcopy(system)
        optimize(on, opt_spec)
        assert recorder.counts() == OBJECTS
        arrays, array_calls = solve_arrays(copy.deepcopy(system), opt_spec, optimize)
        assert array_calls == 1
        python = solve_python(copy.deepcopy(system), opt_spec, optimize)
        assert exported(on)[0], "nothing was allocated"
        assert exported(on) == exported(arrays) == exported(python)
    finally:
        faulthandler.cancel_dump_traceback_later()
