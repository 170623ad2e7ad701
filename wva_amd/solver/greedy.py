"""Greedy capacity-constrained solver (limited mode).

Parity with /root/reference/pkg/solver/greedy.go: per-server sorted
allocation lists; entries ordered by (priority, regret-delta to next-best,
current value); greedy grant, else advance index and binary-search reinsert;
leftover servers get best-effort allocation per saturation policy.

Ordering invariants preserved exactly:
- entries sort by priority ascending, then delta *descending* (largest
  regret first), then current-allocation value *descending*
  (greedy.go:72-83);
- on a capacity miss the entry's index advances and its delta becomes the
  gap to the next-best allocation, or +inf for the last choice
  (greedy.go:147-163);
- best-effort policies may scale an allocation's replica count and rescale
  cost/value by the replica factor (greedy.go:208-211,299-310).

solve_greedy runs the solve itself in C++ (csrc/greedy_core.h) when an
extension carries it: the binding reads the candidates' fields from the
servers' Allocation objects itself (_solve_objects) and returns the chosen
allocation and the granted replicas per server, and _apply sets them,
rescaling partial grants in Python floats.  Whatever that entry point does
not take (an Allocation subclass, a numpy scalar, a bound) goes to _marshal,
which lays the problem out as flat arrays or sends it on to the Python body,
as it did before the binding read objects.  The Python
functions below are unchanged; they are the fallback and the reference the
native route is tested against (docs/design/native-greedy.md).
"""

from __future__ import annotations

import math
import os
from array import array
from typing import Dict, List, Optional

from ..config import OptimizerSpec, SaturationPolicy
from ..core import Allocation, Model, System


class ServerEntry:
    __slots__ = ("server_name", "priority", "cur_index", "allocations", "delta")

    def __init__(self, server_name: str, priority: int, allocations: List[Allocation]) -> None:
        self.server_name = server_name
        self.priority = priority
        self.cur_index = 0
        self.allocations = allocations
        self.delta = 0.0

    def __repr__(self) -> str:
        return (
            f"sName={self.server_name}, prio={self.priority}, curIndex={self.cur_index}, "
            f"delta={self.delta}, allocations={self.allocations}"
        )


def _order_cmp(a: ServerEntry, b: ServerEntry) -> int:
    """Straight priorities, then regret deltas (descending), then current
    value (descending)."""
    if a.priority != b.priority:
        return -1 if a.priority < b.priority else 1
    if a.delta != b.delta:
        return -1 if b.delta < a.delta else 1
    av = a.allocations[a.cur_index].value
    bv = b.allocations[b.cur_index].value
    if av == bv:
        return 0
    return -1 if bv < av else 1


def _insort(entries: List[ServerEntry], entry: ServerEntry) -> None:
    """Insert keeping the _order_cmp ordering (leftmost position with
    cmp(entries[i], entry) >= 0, mirroring slices.BinarySearchFunc)."""
    lo, hi = 0, len(entries)
    while lo < hi:
        mid = (lo + hi) // 2
        if _order_cmp(entries[mid], entry) < 0:
            lo = mid + 1
        else:
            hi = mid
    entries.insert(lo, entry)


_POLICY_CODE = {  # greedy_core.h: Policy
    SaturationPolicy.NONE: 0,
    SaturationPolicy.PRIORITY_EXHAUSTIVE: 1,
    SaturationPolicy.PRIORITY_ROUND_ROBIN: 2,
    SaturationPolicy.ROUND_ROBIN: 3,
}

# bounds that keep every integer of the native solve inside int64: with
# |num_replicas| < 2**31, |units_per_replica| < 2**12 and fewer than 2**18
# allocations the units ever asked for sum to less than 2**61, and so may
# the capacities
_MAX_REPLICAS = 1 << 31
_MAX_UNITS = 1 << 12
_MAX_ALLOCATIONS = 1 << 18
_MAX_CAPACITY = 1 << 61

_UNSET = object()
_binding_module = _UNSET


def _binding():
    """The native module that carries greedy_solve (the torch-free one
    first), or None."""
    global _binding_module
    if _binding_module is _UNSET:
        _binding_module = None
        try:
            from .. import ops
        except Exception:  # pragma: no cover - no numpy in the environment
            return None
        for mod in (ops._native_cpu, ops._native):
            if mod is not None and getattr(mod, "HAS_GREEDY", False):
                _binding_module = mod
                break
    return _binding_module


def _marshal(system: System):
    """One pass over the servers: clear their allocations and lay the
    problem out as the flat arrays of csrc/greedy_core.h.  Returns
    (array arguments, servers, all candidates, their offsets), or None when the
    system has to take the Python body: a missing model, a non-finite value,
    or an integer outside the bounds above."""
    accelerators = system.accelerators
    models = system.models
    type_index: Dict[str, int] = {}
    for acc in accelerators.values():
        type_index.setdefault(acc.type, len(type_index))
    capacity = [0] * len(type_index)
    for t, count in system.capacity.items():
        i = type_index.get(t)
        if i is not None:
            capacity[i] = count

    priorities: Dict[str, int] = {}  # per service class
    servers = list(system.servers.values())
    flat: List[Allocation] = []  # every server's candidates, in order
    model_of: List[str] = []  # per candidate
    priority = []
    offsets = [0]
    for server in servers:
        server.remove_allocation()
        allocs = server.all_allocations
        if allocs:
            model_name = server.model_name
            if model_name not in models:
                return None
            class_name = server.service_class_name
            prio = priorities.get(class_name)
            if prio is None:
                prio = priorities[class_name] = server.priority(system)
            priority.append(prio)
            flat += allocs.values()
            model_of += [model_name] * len(allocs)
        else:
            priority.append(0)
        offsets.append(len(flat))

    values = [a.value for a in flat]
    replicas = [a.num_replicas for a in flat]
    names = [a.accelerator for a in flat]
    # accelerator type and units per replica, resolved once per accelerator
    # and once per (model, accelerator)
    type_of: Dict[str, int] = {}
    for name in set(names):
        acc = accelerators.get(name)
        type_of[name] = -1 if acc is None else type_index[acc.type]
    pairs = list(zip(model_of, names))
    units_of: Dict[tuple, int] = {}
    for pair in set(pairs):
        acc = accelerators.get(pair[1])
        units_of[pair] = (
            0 if acc is None else models[pair[0]].get_num_instances(pair[1]) * acc.multiplicity
        )
    types = [type_of[name] for name in names]
    units = [units_of[pair] for pair in pairs]

    if len(values) >= _MAX_ALLOCATIONS:
        return None
    try:
        if values:
            if not math.isfinite(sum(values)):  # a NaN or an infinity, or a sum that overflows
                return None
            if not (-_MAX_REPLICAS < min(replicas) and max(replicas) < _MAX_REPLICAS):
                return None
            resolved = units_of.values()
            if not (-_MAX_UNITS < min(resolved) and max(resolved) < _MAX_UNITS):
                return None
        if sum(map(abs, capacity)) >= _MAX_CAPACITY:
            return None
        # 'q' and 'i' take nothing but integers that fit; 'd' takes numbers
        args = (
            array("q", capacity), array("q", priority), array("q", offsets),
            array("d", values), array("q", replicas), array("i", types),
            array("q", units),
        )
    except (TypeError, OverflowError):
        return None
    return args, servers, flat, offsets


def _apply(servers, flat, offsets, chosen: List[int], granted: List[int]) -> None:
    """Set what the native solve chose; a partial grant is rescaled here, in
    Python floats, exactly as _allocate_maximally and _allocate_equally do."""
    for server, first, index, count in zip(servers, offsets, chosen, granted):
        if index < 0:
            continue
        alloc = flat[first + index]
        cur = alloc.num_replicas
        if count != cur:
            factor = count / cur
            alloc.cost *= factor
            alloc.value *= factor
            alloc.num_replicas = count
        server.set_allocation(alloc)


def _solve_objects(system: System, spec: OptimizerSpec, binding) -> bool:
    """The native solve with the candidates' fields read inside the binding
    (csrc/greedy_py.h: greedy_solve_objects).  Python builds what is small:
    the priority per server, the capacity per type, the type index per
    accelerator and the units per (model, accelerator) pair that exists.
    False when the binding, or a check here, leaves the decision to
    _marshal; every server's allocation has been cleared by then."""
    accelerators = system.accelerators
    type_index: Dict[str, int] = {}
    types: Dict[str, int] = {}
    for name, acc in accelerators.items():
        types[name] = type_index.setdefault(acc.type, len(type_index))
    capacity = [0] * len(type_index)
    for t, count in system.capacity.items():
        i = type_index.get(t)
        if i is not None:
            capacity[i] = count
    units: Dict[str, Dict[str, int]] = {}
    for name, model in system.models.items():
        if type(model) is not Model:
            return False
        units[name] = {
            a: model.get_num_instances(a) * accelerators[a].multiplicity
            for a in model.num_instances if a in accelerators
        }

    priorities: Dict[str, int] = {}  # per service class
    servers = list(system.servers.values())
    priority = []
    for server in servers:
        server.remove_allocation()
        prio = 0
        if server.all_allocations:
            class_name = server.service_class_name
            prio = priorities.get(class_name)
            if prio is None:
                prio = priorities[class_name] = server.priority(system)
        priority.append(prio)
    try:
        if sum(map(abs, capacity)) >= _MAX_CAPACITY:
            return False
        capacity_arr = array("q", capacity)
    except (TypeError, OverflowError):
        return False
    solved = binding.greedy_solve_objects(
        servers, priority, capacity_arr, types, units, Allocation,
        bool(spec.delayed_best_effort),
        _POLICY_CODE[SaturationPolicy.parse(spec.saturation_policy)],
    )
    if solved is None:
        return False
    chosen, granted, flat, offsets = solved
    _apply(servers, flat, offsets, chosen, granted)
    return True


def _solve_native(system: System, spec: OptimizerSpec, binding) -> bool:
    if getattr(binding, "HAS_GREEDY_OBJECTS", False) and _solve_objects(system, spec, binding):
        return True
    marshalled = _marshal(system)
    if marshalled is None:
        return False
    args, servers, flat, offsets = marshalled
    chosen, granted = binding.greedy_solve(
        *args,
        bool(spec.delayed_best_effort),
        _POLICY_CODE[SaturationPolicy.parse(spec.saturation_policy)],
    )
    _apply(servers, flat, offsets, chosen, granted)
    return True


def solve_greedy(system: System, spec: OptimizerSpec) -> None:
    # native route (csrc/greedy_core.h); WVA_NATIVE_GREEDY=0 switches it off
    if os.environ.get("WVA_NATIVE_GREEDY", "1") != "0":
        binding = _binding()
        if binding is not None and _solve_native(system, spec, binding):
            return

    available: Dict[str, int] = dict(system.capacity)

    entries: List[ServerEntry] = []
    for server_name, server in system.servers.items():
        server.remove_allocation()
        all_allocs = server.all_allocations
        if not all_allocs:
            continue
        allocs = sorted(all_allocs.values(), key=lambda a: a.value)
        e = ServerEntry(server_name, server.priority(system), allocs)
        if len(allocs) > 1:
            e.delta = allocs[1].value - allocs[0].value
        else:
            e.delta = math.inf
        entries.append(e)

    # same ordering as _order_cmp — (priority asc, regret delta desc,
    # current value desc) — as a key tuple: ~10x cheaper than the
    # cmp_to_key wrapper, and equally stable for ties
    entries.sort(
        key=lambda e: (e.priority, -e.delta, -e.allocations[e.cur_index].value)
    )

    if spec.delayed_best_effort:
        unallocated = _allocate(system, entries, available)
        _best_effort(system, unallocated, available, spec.saturation_policy)
    else:
        for group in make_priority_groups(entries):
            unallocated = _allocate(system, group, available)
            _best_effort(system, unallocated, available, spec.saturation_policy)


def _allocate(
    system: System, entries: List[ServerEntry], available: Dict[str, int]
) -> List[ServerEntry]:
    """Greedy SLO-satisfying allocation; returns entries that got nothing."""
    entries = list(entries)
    unallocated: List[ServerEntry] = []
    while entries:
        top = entries.pop(0)
        if not top.allocations:
            continue
        server = system.server(top.server_name)
        if server is None:
            continue
        model = system.model(server.model_name)
        if model is None:
            continue
        alloc = top.allocations[top.cur_index]
        acc = system.accelerator(alloc.accelerator)
        if acc is None:
            continue
        t_name = acc.type
        units_per_replica = model.get_num_instances(alloc.accelerator) * acc.multiplicity
        count = alloc.num_replicas * units_per_replica

        if available.get(t_name, 0) >= count:
            available[t_name] = available.get(t_name, 0) - count
            server.set_allocation(alloc)
        else:
            top.cur_index += 1
            if top.cur_index + 1 < len(top.allocations):
                top.delta = (
                    top.allocations[top.cur_index + 1].value
                    - top.allocations[top.cur_index].value
                )
            elif top.cur_index == len(top.allocations):
                unallocated.append(top)
                continue
            else:
                top.delta = math.inf
            _insort(entries, top)
    return unallocated


def _best_effort(
    system: System,
    unallocated: List[ServerEntry],
    available: Dict[str, int],
    policy: str,
) -> None:
    p = SaturationPolicy.parse(policy)
    if p is SaturationPolicy.PRIORITY_EXHAUSTIVE:
        _allocate_maximally(system, unallocated, available)
    elif p is SaturationPolicy.PRIORITY_ROUND_ROBIN:
        for group in make_priority_groups(unallocated):
            _allocate_equally(system, group, available)
    elif p is SaturationPolicy.ROUND_ROBIN:
        _allocate_equally(system, unallocated, available)
    # SaturationPolicy.NONE: no allocation beyond satisfying SLOs


def _allocate_maximally(
    system: System, entries: List[ServerEntry], available: Dict[str, int]
) -> None:
    """Priority ordering: one server at a time exhaustively."""
    for entry in entries:
        for alloc in entry.allocations:
            acc_name = alloc.accelerator
            server = system.server(entry.server_name)
            if server is None:
                continue
            model = system.model(server.model_name)
            acc = system.accelerator(acc_name)
            if acc is None or model is None:
                continue
            units_per_replica = model.get_num_instances(acc_name) * acc.multiplicity
            if units_per_replica <= 0:
                continue
            max_replicas = available.get(acc.type, 0) // units_per_replica
            max_replicas = min(max_replicas, alloc.num_replicas)
            if max_replicas > 0:
                cur = alloc.num_replicas
                factor = max_replicas / cur
                alloc.cost *= factor
                alloc.value *= factor
                alloc.num_replicas = max_replicas
                server.set_allocation(alloc)
                available[acc.type] = available.get(acc.type, 0) - max_replicas * units_per_replica
                break


class _Ticket:
    __slots__ = ("entry", "active", "server", "model", "acc_type", "units_per_replica", "num_replicas", "final_alloc")

    def __init__(self, entry: ServerEntry, server, model) -> None:
        self.entry = entry
        self.active = False
        self.server = server
        self.model = model
        self.acc_type = ""
        self.units_per_replica = 0
        self.num_replicas = 0
        self.final_alloc: Optional[Allocation] = None


def _allocate_equally(
    system: System, entries: List[ServerEntry], available: Dict[str, int]
) -> None:
    """Round-robin: one replica per visit until capacity runs out."""
    tickets: Dict[str, _Ticket] = {}
    for entry in entries:
        server = system.server(entry.server_name)
        if server is None:
            continue
        model = system.model(server.model_name)
        if model is None:
            continue
        tickets[entry.server_name] = _Ticket(entry, server, model)

    allocated: Dict[str, _Ticket] = {}
    while tickets:
        for entry in entries:
            ticket = tickets.get(entry.server_name)
            if ticket is None:
                continue
            if not ticket.active:
                for alloc in entry.allocations:
                    acc = system.accelerator(alloc.accelerator)
                    if acc is None:
                        continue
                    units = ticket.model.get_num_instances(alloc.accelerator) * acc.multiplicity
                    if units > 0 and available.get(acc.type, 0) >= units:
                        ticket.active = True
                        ticket.acc_type = acc.type
                        ticket.units_per_replica = units
                        ticket.final_alloc = alloc
                        break
                if not ticket.active:
                    del tickets[entry.server_name]
                    continue
            replicas_available = available.get(ticket.acc_type, 0) // ticket.units_per_replica
            if min(replicas_available, ticket.final_alloc.num_replicas) > 0:
                ticket.num_replicas += 1
                available[ticket.acc_type] = available.get(ticket.acc_type, 0) - ticket.units_per_replica
                allocated[entry.server_name] = ticket
            else:
                del tickets[entry.server_name]

    for ticket in allocated.values():
        alloc = ticket.final_alloc
        cur = alloc.num_replicas
        factor = ticket.num_replicas / cur
        alloc.cost *= factor
        alloc.value *= factor
        alloc.num_replicas = ticket.num_replicas
        ticket.server.set_allocation(alloc)


def make_priority_groups(entries: List[ServerEntry]) -> List[List[ServerEntry]]:
    """Partition an ordered entry list into runs of equal priority."""
    groups: List[List[ServerEntry]] = []
    i, n = 0, len(entries)
    while i < n:
        group = [entries[i]]
        prio = entries[i].priority
        i += 1
        while i < n and entries[i].priority == prio:
            group.append(entries[i])
            i += 1
        groups.append(group)
    return groups
