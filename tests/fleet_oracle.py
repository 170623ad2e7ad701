"""Fleet-level oracle: whole systems whose sizing cycle has a known answer.

test_ops_oracle*.py hold the ``[B, 12] -> [B, 6]`` matrix solve to the exact
oracle.  This module does the same for the layer above it — ``System`` ->
rows -> ``Allocation`` objects -> ``Manager.optimize()`` — which is what
``BatchedAllocationSolver.calculate()`` and the benchmark actually run.

A fleet is a seeded ``SystemSpec`` plus, for every (server, candidate
accelerator) pair, what the cycle must produce:

- the problem row, built by ``expected_row`` from the *definitions* in
  core/allocation.py's docstring and ``create_allocation`` (N rule, token
  truncation, total rate and headroom, min replicas) — never from
  ``build_rows``;
- the oracle's solve of that row (``mm1k_oracle.oracle_solve``): feasibility,
  replicas, ``rate_star``, final ITL/TTFT/rho, with ``rate_tol`` and the
  per-row ``final_tol = row_bound(scale)`` exactly as test_ops_oracle_wide.py
  derives them;
- cost ``= acc.cost * (instances * replicas)``, the value under the cost
  objective (cost, or the transition penalty against the current
  allocation) and, for ``cost+energy``, the energy term from the oracle's rho
  with its bound ``final_tol * max_slope / idle_power``.

Pairs the solver never sees (zero load; missing model, class, target or perf
data) take their expectation from the scalar path, bit for bit; this module
only records which pairs those are.

A server is redrawn when the oracle drops any of its pairs (a correct float64
solver could decide them differently); the reason is counted, and at most
MAX_DROP_SHARE of the drawn servers may go.  A kept fleet therefore has no
ambiguous pair and every assertion made on it is unconditional.

Helper module (like mm1k_oracle.py and fixtures.py), not a conftest.
"""

from __future__ import annotations

import copy
import time
from collections import Counter
from typing import Dict, List, NamedTuple, Optional

import numpy as np

import mm1k_oracle as oracle
from test_ops_oracle_wide import MAX_DROP_SHARE, row_bound
from wva_amd.config import (
    AcceleratorCount,
    AcceleratorData,
    AcceleratorSpec,
    AllocationData,
    CapacityData,
    DecodeParmsSpec,
    ModelAcceleratorPerfData,
    ModelData,
    ModelTarget,
    OptimizerData,
    OptimizerSpec,
    PowerSpec,
    PrefillParmsSpec,
    ServerData,
    ServerLoadSpec,
    ServerSpec,
    ServiceClassData,
    ServiceClassSpec,
    SystemSpec,
)

# one seed per random fleet; chosen so that the redraw share stays under
# MAX_DROP_SHARE (asserted in build_fleets)
RANDOM_SEEDS = tuple(range(7100, 7124))
HEADROOM = 0.25  # the fleets that run with WVA_SIZING_HEADROOM set

INSTANCE_COUNTS = (1, 2, 3, 4, 6, 8)
SERVER_MAX_BATCH = (0, 1, 8, 64)  # 0: N falls back to the perf data
POLICIES = ("None", "PriorityExhaustive", "PriorityRoundRobin", "RoundRobin")
ACCEL_PENALTY = 0.1  # allocation.py docstring: 0.1 * (costA + costB) on a type change
ORACLE_MAX_N = 64  # random fleets stay at or below it so the oracle stays cheap
ENERGY_PRICE = 12.5  # cents per kWh in the cost+energy fleets

# minimum coverage over all fleets (build_fleets asserts each)
MIN_COVERAGE = {
    "ttft-bound": 15, "itl-bound": 15, "at a cap": 15, "infeasible": 15,
    "zero-load": 10, "fallback-N": 30, "non-dyadic cost x odd instances": 30,
    "skipped": 10, "with penalty": 50,
}

# (cost1, instances1, cost2, instances2, replicas): cost1 * instances1 ==
# cost2 * instances2 exactly, and at this replica count the two float
# associations cost * (instances * replicas) and (cost * instances) * replicas
# order the two accelerators differently.  The first two are the "three small
# cards for the price of one big one" price list; the others were found by
# enumerating two-decimal prices.  "scalar_tie": the definition's association
# ties (first accelerator wins), the other makes the second one cheaper;
# "scalar_strict": the definition makes the second one cheaper, the other
# association ties or reverses.  build_tie_fleet re-checks each in floats.
TIES = (
    ("scalar_tie", 2.1, 1, 0.7, 3, 5),
    ("scalar_tie", 2.1, 1, 0.7, 3, 10),
    ("scalar_tie", 6.4, 3, 2.4, 8, 5),
    ("scalar_tie", 10.8, 3, 32.4, 1, 10),
    ("scalar_strict", 12.48, 3, 9.36, 4, 6),
    ("scalar_strict", 57.39, 8, 76.52, 6, 3),
)


class Pair(NamedTuple):
    """What the cycle must produce for one (server, accelerator) pair."""

    server: str
    acc: str
    kind: str  # "solved" | "zero_load"
    case: Optional[dict]  # oracle case of a solved pair (test_ops_oracle.oracle_errors)
    batch_size: int
    fallback_n: bool
    cost: float  # acc.cost * (instances * replicas)
    value: float  # under the cost objective
    energy: float  # expected energy term (0 unless the fleet's objective has one)
    energy_tol: float  # absolute bound on the energy part of the value


class Fleet:
    def __init__(self, name, spec, headroom=None):
        self.name = name
        self.spec = spec
        self.headroom = headroom  # None: WVA_SIZING_HEADROOM unset
        self.pairs: Dict[str, List[Pair]] = {}  # per server, in candidate order
        self.skipped = Counter()  # reason -> pairs (or whole servers) without a row
        self.redrawn = Counter()  # oracle drop reason -> servers redrawn
        self.drawn = 0
        self.variants: List[tuple] = []  # (label, OptimizerSpec, capacity {type: count})

    @property
    def energy(self) -> bool:
        o = self.spec.optimizer.spec
        return o.objective == "cost+energy" and o.energy_cost_per_kwh > 0

    def solved_pairs(self):
        return [p for ps in self.pairs.values() for p in ps if p.kind == "solved"]

    def rows(self) -> int:
        return len(self.solved_pairs())

    def __repr__(self):
        return f"Fleet({self.name})"


# ---------------------------------------------------------------------------
# The definitions, written out independently of wva_amd.ops.batched
# ---------------------------------------------------------------------------

def _perf_of(spec: SystemSpec, model: str, acc: str):
    found = None
    for pd in spec.models.perf_data:
        if pd.name == model and pd.acc == acc:
            found = pd  # a later entry replaces an earlier one
    return found


def _instances(pd) -> int:
    return pd.acc_count if pd.acc_count > 0 else 1


def _target_of(spec: SystemSpec, class_name: str, model: str):
    """(status, ModelTarget): status names what is missing, or is None."""
    if not any(pd.name == model for pd in spec.models.perf_data):
        return "missing_model", None
    for sc in spec.service_classes.spec:
        if sc.name == class_name:
            found = None
            for mt in sc.model_targets:
                if mt.model == model:
                    found = mt
            return (None, found) if found is not None else ("missing_target", None)
    return "missing_class", None


def candidates_of(spec: SystemSpec, server: ServerSpec) -> List[AcceleratorSpec]:
    """Candidate accelerators in enumeration order: all of them in spec
    order, or only the current one for a keep-accelerator server."""
    accs = list(spec.accelerators.spec)
    if server.keep_accelerator and server.current_alloc.accelerator:
        return [a for a in accs if a.name == server.current_alloc.accelerator]
    return accs


def expected_row(spec: SystemSpec, server: ServerSpec, acc: AcceleratorSpec, headroom=None):
    """The sizing row of one pair, from the definitions.

    Returns ("skip", reason), ("zero_load", None) or ("row", (row, N,
    fallback)).  N is the server's max batch size, or without one
    max(perf.maxBatchSize * atTokens // K, 1); K = int(out_tokens); the input
    tokens are truncated the same way; the total rate is arrival / 60 (req/min
    -> req/s), or TPS / K under a TPS target, times 1 + headroom."""
    load = server.current_alloc.load
    if load is None or load.arrival_rate < 0 or load.avg_in_tokens < 0 or load.avg_out_tokens < 0:
        return "skip", "bad_load"
    status, target = _target_of(spec, server.class_name, server.model)
    if status is not None:
        return "skip", status
    pd = _perf_of(spec, server.model, acc.name)
    if pd is None:
        return "skip", "missing_perf"
    if load.arrival_rate == 0 or load.avg_out_tokens == 0:
        return "zero_load", None
    k = int(load.avg_out_tokens)
    fallback = not server.max_batch_size > 0
    if k == 0 and not fallback:
        # 0 < out_tokens < 1: the analyzer rejects a request without a whole
        # output token before anything divides by K
        return "skip", "under_one_output_token"
    n = max(pd.max_batch_size * pd.at_tokens // k, 1) if fallback else server.max_batch_size
    if target.slo_tps == 0:
        total = load.arrival_rate / 60.0
    else:
        total = target.slo_tps / float(k)
    total *= 1.0 + (headroom or 0.0)
    row = np.array(
        [pd.decode_parms.alpha, pd.decode_parms.beta, pd.prefill_parms.gamma,
         pd.prefill_parms.delta, float(int(load.avg_in_tokens)), float(k), float(n),
         target.slo_ttft, target.slo_itl, target.slo_tps, total, float(server.min_num_replicas)],
        dtype=np.float64,
    )
    return "row", (row, n, fallback)


def expected_penalty(cur: AllocationData, acc_name: str, replicas: int, cost: float) -> float:
    """Transition penalty from the current allocation to (acc, replicas,
    cost): nothing for the same allocation, the cost delta on the same
    accelerator, and 0.1 * (costA + costB) on top of it on a change."""
    if cur.accelerator == acc_name:
        return 0.0 if cur.num_replicas == replicas else cost - cur.cost
    return ACCEL_PENALTY * (cur.cost + cost) + (cost - cur.cost)


def power_of(p: PowerSpec, util: float) -> float:
    """Piecewise-linear power curve: idle -> midPower at midUtil -> full."""
    if util <= p.mid_util:
        return p.idle + (p.mid_power - p.idle) / p.mid_util * util
    return p.mid_power + (p.full - p.mid_power) / (1.0 - p.mid_util) * (util - p.mid_util)


def max_power_slope(p: PowerSpec) -> float:
    return max((p.mid_power - p.idle) / p.mid_util, (p.full - p.mid_power) / (1.0 - p.mid_util))


_solve_cache: Dict[bytes, tuple] = {}


def _oracle_solve(row):
    key = row.tobytes()
    hit = _solve_cache.get(key)
    if hit is None:
        case, reason = oracle.oracle_solve(row)
        if case is not None and case["feasible"]:
            case["final_tol"] = row_bound(case["scale"])
            if case["rate_tol"] is None:  # lam is a cap: known exactly
                case["rate_tol"] = case["final_tol"]
        hit = _solve_cache[key] = (case, reason)
    return hit


def server_pairs(spec: SystemSpec, server: ServerSpec, headroom, energy_price=0.0):
    """(pairs, skipped reasons, None) of one server, or (None, None, reason)
    when the oracle drops one of its pairs."""
    pairs, skipped = [], Counter()
    candidates = candidates_of(spec, server)
    if not candidates:
        skipped["no_candidate"] += 1
    for acc in candidates:
        what, payload = expected_row(spec, server, acc, headroom)
        if what == "skip":
            skipped[payload] += 1
            continue
        if what == "zero_load":
            pairs.append(Pair(server.name, acc.name, "zero_load", None, 0, False, 0.0, 0.0, 0.0, 0.0))
            continue
        row, n, fallback = payload
        case, reason = _oracle_solve(row)
        if case is None:
            return None, None, reason
        cost = value = energy = energy_tol = 0.0
        if case["feasible"]:
            pd = _perf_of(spec, server.model, acc.name)
            replicas = case["replicas"]
            cost = acc.cost * (_instances(pd) * replicas)
            value = expected_penalty(server.current_alloc, acc.name, replicas, cost)
            if energy_price > 0:
                cards = _instances(pd) * acc.multiplicity * replicas
                energy = power_of(acc.power, float(case["final"].rho)) * cards / 1000.0 * energy_price
                energy_tol = energy * case["final_tol"] * max_power_slope(acc.power) / acc.power.idle
        pairs.append(Pair(server.name, acc.name, "solved", case, n, fallback, cost, value,
                          energy, energy_tol))
    return pairs, skipped, None


# ---------------------------------------------------------------------------
# Seeded generator
# ---------------------------------------------------------------------------

ACC_NAMES = ("MI355X", "MI325X", "MI300X", "L40S")
ACC_TYPES = ("AMD-MI355X-288GB", "AMD-MI3xx-pool", "AMD-MI3xx-pool", "EMU-L40S-48GB")
MODEL_NAMES = ("llama-8b", "llama-70b", "mixtral-8x7b")
CLASS_NAMES = ("Premium", "Standard", "Freemium")


def _draw_accelerators(rng, n_acc):
    """The pooled pair (one shared type) is always among them."""
    keep = [1, 2] + [int(i) for i in rng.permutation([0, 3])[: n_acc - 2]]
    accs = []
    for i in sorted(keep):
        idle = int(rng.integers(30, 160))
        mid = idle + int(rng.integers(100, 600))
        accs.append(AcceleratorSpec(
            name=ACC_NAMES[i], type=ACC_TYPES[i], multiplicity=int(rng.choice((1, 2))),
            mem_size=192, mem_bw=5300,
            power=PowerSpec(idle=idle, full=mid + int(rng.integers(100, 600)), mid_power=mid,
                            mid_util=float(rng.choice((0.5, 0.6, 0.7)))),
            cost=round(float(rng.uniform(0.5, 120)), 2),
        ))
    order = rng.permutation(len(accs))
    return [accs[i] for i in order]


def _draw_perf(rng, models, accs):
    perf = []
    for m in models:
        have = 0
        for j, acc in enumerate(accs):
            if rng.random() < 0.15 and not (j == len(accs) - 1 and have == 0):
                continue  # no perf data for this pair
            have += 1
            perf.append(ModelAcceleratorPerfData(
                name=m, acc=acc.name, acc_count=int(rng.choice(INSTANCE_COUNTS)),
                # small enough that the fallback N = mbs * at // K stays
                # within ORACLE_MAX_N for K >= 32, and reaches the clamp at 1
                max_batch_size=int(rng.choice((4, 8, 16))),
                at_tokens=int(rng.choice((32, 64, 128))),
                decode_parms=DecodeParmsSpec(alpha=float(rng.uniform(2, 25)),
                                             beta=float(rng.uniform(0.005, 0.5))),
                prefill_parms=PrefillParmsSpec(gamma=float(rng.uniform(2, 60)),
                                               delta=float(rng.uniform(0.001, 0.2))),
            ))
    return perf


def _itl_target(rng, perf, model, batch_sizes):
    """An ITL target some pair of this model can actually be bound by: the
    decode time alpha + beta * b of one of its profiles at a batch size
    within the reach of the drawn batch limits.  Profiles with a larger
    alpha find it infeasible, faster ones never reach it."""
    own = [pd for pd in perf if pd.name == model]
    pd = own[int(rng.integers(0, len(own)))]
    b = float(rng.uniform(0.4, 1.1)) * float(rng.choice(batch_sizes))
    return pd.decode_parms.alpha + pd.decode_parms.beta * max(b, 1.2)


def _draw_classes(rng, n_classes, models, perf):
    priorities = [int(rng.integers(1, 4))] * 2 + [int(rng.integers(4, 20))]
    masks = [int(m) for m in rng.permutation(8)]  # which of ttft/itl/tps are 0
    lacking = (int(rng.integers(0, n_classes)), int(rng.integers(0, len(models))))
    classes, t = [], 0
    for c in range(n_classes):
        targets = []
        for mi, m in enumerate(models):
            if (c, mi) == lacking:
                continue  # this class has no target for this model
            mask = masks[t % 8]
            t += 1
            targets.append(ModelTarget(
                model=m,
                slo_ttft=0.0 if mask & 1 else float(10 ** rng.uniform(1.6, 4.5)),
                slo_itl=0.0 if mask & 2 else _itl_target(rng, perf, m, (4, 8, 32, 64)),
                slo_tps=0.0 if mask & 4 else float(rng.uniform(50, 3000)),
            ))
        classes.append(ServiceClassSpec(name=CLASS_NAMES[c], priority=priorities[c],
                                        model_targets=targets))
    return classes


def _min_fallback_k(perf, model):
    """Smallest K at which every fallback N of this model is <= ORACLE_MAX_N."""
    worst = max((pd.max_batch_size * pd.at_tokens for pd in perf if pd.name == model), default=1)
    return -(-worst // ORACLE_MAX_N)


def _draw_server(rng, name, accs, perf, models, classes):
    model = str(rng.choice(models))
    class_name = str(rng.choice([c.name for c in classes]))
    u = rng.random()
    if u < 0.03:
        model = "no-such-model"
    elif u < 0.06:
        class_name = "no-such-class"
    max_batch = int(rng.choice(SERVER_MAX_BATCH))
    arrival = 0.0 if rng.random() < 0.12 else float(10 ** rng.uniform(0.5, 4))  # req/min
    u = rng.random()
    if u < 0.1:
        in_tokens = 0
    elif u < 0.3:
        in_tokens = float(rng.uniform(1, 2000))  # fractional: truncated
    else:
        in_tokens = int(rng.integers(1, 2049))
    u = rng.random()
    if max_batch == 0:
        # the fallback N divides by K: keep it within the oracle's budget
        lo = max(_min_fallback_k(perf, model), 1)
        out_tokens = float(rng.uniform(lo, 600)) if u < 0.3 else int(rng.integers(lo, 601))
    elif u < 0.06:
        out_tokens = 0
    elif u < 0.16:
        out_tokens = 1
    elif u < 0.36:
        out_tokens = float(rng.uniform(1, 600))  # fractional >= 1: truncated
    else:
        out_tokens = int(rng.integers(2, 601))
    cur = AllocationData(load=ServerLoadSpec(arrival_rate=arrival, avg_in_tokens=in_tokens,
                                             avg_out_tokens=out_tokens))
    keep = rng.random() < 0.15
    if keep or rng.random() < 0.5:
        cur.accelerator = str(rng.choice([a.name for a in accs]))
        cur.num_replicas = int(rng.integers(1, 7))
        cur.max_batch = max_batch
        cur.cost = round(float(rng.uniform(1, 2000)), 2)
    return ServerSpec(name=name, class_name=class_name, model=model, keep_accelerator=keep,
                      min_num_replicas=int(rng.integers(0, 4)), max_batch_size=max_batch,
                      current_alloc=cur)


def _fill_servers(fleet: Fleet, draw_one, n_servers, energy_price=0.0):
    """Draw servers until n_servers are kept; a server is redrawn when the
    oracle drops any of its pairs."""
    kept = []
    while len(kept) < n_servers:
        fleet.drawn += 1
        assert fleet.drawn <= 4 * n_servers + 8, f"{fleet.name}: redraws do not converge"
        server = draw_one(len(kept), fleet.drawn)
        pairs, skipped, reason = server_pairs(fleet.spec, server, fleet.headroom, energy_price)
        if pairs is None:
            fleet.redrawn[reason] += 1
            continue
        kept.append(server)
        fleet.pairs[server.name] = pairs
        fleet.skipped.update(skipped)
    fleet.spec.servers.spec.extend(kept)


def units_demanded(fleet: Fleet) -> Dict[str, int]:
    """Per accelerator type, the cards the fleet would take if every server
    got its largest feasible candidate of that type."""
    accs = {a.name: a for a in fleet.spec.accelerators.spec}
    demand: Dict[str, int] = {a.type: 0 for a in accs.values()}
    servers = {s.name: s for s in fleet.spec.servers.spec}
    for name, pairs in fleet.pairs.items():
        per_type: Dict[str, int] = {}
        for p in pairs:
            if p.kind != "solved" or not p.case["feasible"]:
                continue
            acc = accs[p.acc]
            pd = _perf_of(fleet.spec, servers[name].model, p.acc)
            units = p.case["replicas"] * _instances(pd) * acc.multiplicity
            per_type[acc.type] = max(per_type.get(acc.type, 0), units)
        for t, u in per_type.items():
            demand[t] += u
    return demand


def _optimizer_variants(fleet: Fleet):
    """Unlimited mode, and limited mode under every saturation policy, with
    delayed best effort both ways, on scarce capacity (a third of the demand)
    and on ample capacity (twice the demand)."""
    demand = units_demanded(fleet)
    scarce = {t: u // 3 for t, u in demand.items()}
    ample = {t: 2 * u + 8 for t, u in demand.items()}
    base = fleet.spec.optimizer.spec
    variants = [("unlimited", OptimizerSpec(unlimited=True, objective=base.objective,
                                            energy_cost_per_kwh=base.energy_cost_per_kwh), {})]
    for policy in POLICIES:
        for delayed in (False, True):
            for label, capacity in (("scarce", scarce), ("ample", ample)):
                if label == "ample" and (policy != "None" and delayed):
                    continue  # nothing is left over on ample capacity: one pass per policy
                variants.append((
                    f"{label}-{policy}-{'delayed' if delayed else 'grouped'}",
                    OptimizerSpec(unlimited=False, delayed_best_effort=delayed,
                                  saturation_policy=policy, objective=base.objective,
                                  energy_cost_per_kwh=base.energy_cost_per_kwh),
                    capacity,
                ))
    return variants


def random_fleet(seed: int, index: int) -> Fleet:
    rng = np.random.default_rng(seed)
    accs = _draw_accelerators(rng, int(rng.integers(3, 5)))
    models = list(MODEL_NAMES[: int(rng.integers(2, 4))])
    perf = _draw_perf(rng, models, accs)
    classes = _draw_classes(rng, int(rng.integers(2, 4)), models, perf)
    energy = index % 4 == 3
    # the drawn optimizer; the tests also run every _optimizer_variants entry
    optimizer = OptimizerSpec(
        unlimited=index % 3 == 0,
        delayed_best_effort=bool(index % 2),
        saturation_policy=POLICIES[index % 4],
        objective="cost+energy" if energy else "",
        energy_cost_per_kwh=ENERGY_PRICE if energy else 0.0,
    )
    spec = SystemSpec(
        accelerators=AcceleratorData(spec=accs),
        models=ModelData(perf_data=perf),
        service_classes=ServiceClassData(spec=classes),
        servers=ServerData(spec=[]),
        optimizer=OptimizerData(spec=optimizer),
        capacity=CapacityData(count=[]),
    )
    fleet = Fleet(f"random-{seed}", spec, headroom=HEADROOM if index % 2 else None)
    n_servers = (1, 12)[index] if index < 2 else int(rng.integers(1, 13))
    _fill_servers(
        fleet,
        lambda i, drawn: _draw_server(rng, f"s{i}-{drawn}:ns", accs, perf, models, classes),
        n_servers, ENERGY_PRICE if energy else 0.0,
    )
    fleet.variants = _optimizer_variants(fleet)
    # the drawn capacity: scarce for a third of the fleets, ample otherwise
    by_label = {label: capacity for label, _, capacity in fleet.variants}
    drawn = by_label["scarce-None-grouped" if index % 3 == 1 else "ample-None-grouped"]
    spec.capacity.count = [AcceleratorCount(type=t, count=c) for t, c in drawn.items()]
    fleet.variants.append(("as-drawn", optimizer, dict(drawn)))
    return fleet


# ---------------------------------------------------------------------------
# Named fleets
# ---------------------------------------------------------------------------

def _plain_spec(accs, perf, classes, optimizer=None):
    return SystemSpec(
        accelerators=AcceleratorData(spec=accs),
        models=ModelData(perf_data=perf),
        service_classes=ServiceClassData(spec=classes),
        servers=ServerData(spec=[]),
        optimizer=OptimizerData(spec=optimizer or OptimizerSpec(unlimited=True)),
        capacity=CapacityData(count=[]),
    )


def _loaded_server(rng, name, model, class_name, max_batch, accs, out_lo=2):
    """A server with load (never zero-load, never skipped)."""
    in_tokens = float(rng.uniform(1, 2000)) if rng.random() < 0.2 else int(rng.integers(0, 2049))
    out_tokens = float(rng.uniform(out_lo, 600)) if rng.random() < 0.2 else int(rng.integers(out_lo, 601))
    cur = AllocationData(load=ServerLoadSpec(arrival_rate=float(10 ** rng.uniform(0.5, 4)),
                                             avg_in_tokens=in_tokens, avg_out_tokens=out_tokens))
    if rng.random() < 0.5:
        cur.accelerator = str(rng.choice([a.name for a in accs]))
        cur.num_replicas = int(rng.integers(1, 7))
        cur.cost = round(float(rng.uniform(1, 2000)), 2)
    return ServerSpec(name=name, class_name=class_name, model=model,
                      min_num_replicas=int(rng.integers(0, 4)), max_batch_size=max_batch,
                      current_alloc=cur)


def _named_base(rng, n_acc=4, n_models=2, itl_batches=None):
    """Accelerators, full perf data and two classes with all-target mixes."""
    accs = _draw_accelerators(rng, n_acc)
    models = list(MODEL_NAMES[:n_models])
    perf = _draw_perf(rng, models, accs)
    have = {(pd.name, pd.acc) for pd in perf}
    for m in models:  # these fleets promise a row for every pair
        for acc in accs:
            if (m, acc.name) not in have:
                perf.append(ModelAcceleratorPerfData(
                    name=m, acc=acc.name, acc_count=int(rng.choice(INSTANCE_COUNTS)),
                    max_batch_size=8, at_tokens=64,
                    decode_parms=DecodeParmsSpec(alpha=float(rng.uniform(2, 25)),
                                                 beta=float(rng.uniform(0.005, 0.5))),
                    prefill_parms=PrefillParmsSpec(gamma=float(rng.uniform(2, 60)),
                                                   delta=float(rng.uniform(0.001, 0.2))),
                ))
    classes = [
        ServiceClassSpec(name=CLASS_NAMES[c], priority=1 + 4 * c, model_targets=[
            ModelTarget(model=m, slo_ttft=0.0 if c else float(rng.uniform(200, 3000)),
                        slo_itl=(_itl_target(rng, perf, m, itl_batches) if itl_batches
                                 else float(rng.uniform(5, 30))),
                        slo_tps=0.0 if (c + i) % 2 else float(rng.uniform(50, 3000)))
            for i, m in enumerate(models)])
        for c in range(2)
    ]
    return accs, models, perf, classes


def chip_filling_fleet() -> Fleet:
    """(a) 128 servers x 4 accelerators, every pair a row, all N <= 8: at
    512 rows and more the GPU path takes one launch (no chunking) and the
    launcher picks its 128-thread geometry."""
    rng = np.random.default_rng(8101)
    accs, models, perf, classes = _named_base(rng)
    for pd in perf:  # fallback N = 8 * 64 // K <= 8 for K >= 64
        pd.max_batch_size, pd.at_tokens = 8, 64
    fleet = Fleet("chip-filling-512", _plain_spec(accs, perf, classes))

    def draw(i, drawn):
        max_batch = (0, 1, 8, 4)[i % 4]
        return _loaded_server(rng, f"a{i}-{drawn}:ns", models[i % 2], CLASS_NAMES[(i // 2) % 2],
                              max_batch, accs, out_lo=64 if max_batch == 0 else 2)

    _fill_servers(fleet, draw, 128)
    assert fleet.rows() >= 512 and all(p.batch_size <= 8 for p in fleet.solved_pairs())
    fleet.variants = [v for v in _optimizer_variants(fleet)
                      if v[0] in ("unlimited", "scarce-PriorityRoundRobin-grouped")]
    return fleet


def flagship_chain_fleet() -> Fleet:
    """(b) at most 6 pairs at N = 256, the flagship chain length."""
    rng = np.random.default_rng(8102)
    accs, models, perf, classes = _named_base(rng, n_acc=3, itl_batches=(64, 128))
    fleet = Fleet("flagship-N256", _plain_spec(accs, perf, classes))
    _fill_servers(
        fleet,
        lambda i, drawn: _loaded_server(rng, f"b{i}-{drawn}:ns", models[i % 2], CLASS_NAMES[i % 2],
                                        256, accs),
        2,
    )
    assert 1 <= fleet.rows() <= 6 and all(p.batch_size == 256 for p in fleet.solved_pairs())
    fleet.variants = _optimizer_variants(fleet)[:3]
    return fleet


OVERSIZED_N = 1024  # beyond the GPU's LDS-resident limit (GPU_MAX_BATCH_LIMIT = 700)


def oversized_fleet() -> Fleet:
    """(c) one server with max_batch = 1024 among ordinary ones: on the GPU
    its chunk takes the dispatch's synchronous split to the CPU solver."""
    rng = np.random.default_rng(8103)
    accs, models, perf, classes = _named_base(rng, n_acc=3, itl_batches=(8, 64))
    fleet = Fleet("oversized-N1024", _plain_spec(accs, perf, classes))

    def draw(i, drawn):
        max_batch = OVERSIZED_N if i == 1 else (8, 64, 1)[i % 3]
        return _loaded_server(rng, f"c{i}-{drawn}:ns", models[i % 2], CLASS_NAMES[i % 2],
                              max_batch, accs)

    _fill_servers(fleet, draw, 5)
    assert sum(p.batch_size == OVERSIZED_N for p in fleet.solved_pairs()) == 3
    fleet.variants = _optimizer_variants(fleet)[:3]
    return fleet


def build_tie_fleet(index: int) -> Fleet:
    """(d) two accelerators with identical perf data whose prices tie
    exactly, and a lightly loaded server whose min_replicas puts the two
    float associations of the cost on different sides of the tie."""
    kind, c1, i1, c2, i2, replicas = TIES[index]
    # the property itself, in floats: under the definition's association ...
    s1, s2 = c1 * (i1 * replicas), c2 * (i2 * replicas)
    # ... and under the other one
    o1, o2 = (c1 * i1) * replicas, (c2 * i2) * replicas
    value = lambda cost: ACCEL_PENALTY * (0.0 + cost) + (cost - 0.0)  # noqa: E731
    if kind == "scalar_tie":
        assert value(s1) == value(s2) and value(o2) < value(o1), TIES[index]
    else:
        assert value(s2) < value(s1) and value(o1) <= value(o2), TIES[index]
    power = PowerSpec(idle=130, full=750, mid_power=520, mid_util=0.6)
    accs = [
        AcceleratorSpec(name="MI355X", type="AMD-MI355X-288GB", power=power, cost=c1),
        AcceleratorSpec(name="MI300X", type="AMD-MI300X-192GB", power=power, cost=c2),
    ]
    perf = [
        ModelAcceleratorPerfData(
            name="llama-8b", acc=name, acc_count=count, max_batch_size=8, at_tokens=64,
            decode_parms=DecodeParmsSpec(alpha=6.0, beta=0.05),
            prefill_parms=PrefillParmsSpec(gamma=10.0, delta=0.05))
        for name, count in (("MI355X", i1), ("MI300X", i2))
    ]
    classes = [ServiceClassSpec(name="Premium", priority=1, model_targets=[
        ModelTarget(model="llama-8b", slo_itl=40.0, slo_ttft=2000.0)])]
    fleet = Fleet(f"tie-{index}-{kind}", _plain_spec(accs, perf, classes))
    servers = [
        ServerSpec(name=f"t{j}:ns", class_name="Premium", model="llama-8b",
                   min_num_replicas=replicas, max_batch_size=8,
                   current_alloc=AllocationData(load=ServerLoadSpec(
                       arrival_rate=6.0 + 3.0 * j, avg_in_tokens=128, avg_out_tokens=64)))
        for j in range(2)
    ]
    _fill_servers(fleet, lambda i, drawn: servers[i], 2)
    assert not fleet.redrawn
    for p in fleet.solved_pairs():  # low load: min_replicas decides
        assert p.case["feasible"] and p.case["replicas"] == replicas
    fleet.variants = _optimizer_variants(fleet)[:3]
    return fleet


# ---------------------------------------------------------------------------
# The whole table
# ---------------------------------------------------------------------------

def _dyadic(x: float) -> bool:
    """Whether a two-decimal price is a multiple of 1/4 (exact in binary)."""
    return (x * 4.0).is_integer()


def coverage_of(fleets) -> Dict[str, int]:
    counts = Counter()
    subsets = set()
    for f in fleets:
        accs = {a.name: a for a in f.spec.accelerators.spec}
        servers = {s.name: s for s in f.spec.servers.spec}
        counts["skipped"] += sum(f.skipped.values())
        for name, pairs in f.pairs.items():
            for p in pairs:
                if p.kind == "zero_load":
                    counts["zero-load"] += 1
                    continue
                c = p.case
                row = c["row"]
                subsets.add((row[7] == 0, row[8] == 0, row[9] == 0))
                counts["fallback-N"] += p.fallback_n
                if not c["feasible"]:
                    counts["infeasible"] += 1
                    continue
                counts["ttft-bound"] += c["bound"] == "ttft"
                counts["itl-bound"] += c["bound"] == "itl"
                counts["at a cap"] += c["bound"] in ("tps", "none")
                inst = _instances(_perf_of(f.spec, servers[name].model, p.acc))
                odd = inst & (inst - 1) != 0  # not a power of two
                counts["non-dyadic cost x odd instances"] += odd and not _dyadic(accs[p.acc].cost)
                counts["with penalty"] += bool(servers[name].current_alloc.accelerator)
    counts["target subsets"] = len(subsets)
    return dict(counts)


RANDOM_NAMES = tuple(f"random-{seed}" for seed in RANDOM_SEEDS)
TIE_NAMES = tuple(f"tie-{i}-{t[0]}" for i, t in enumerate(TIES))
CHIP_FILLING, FLAGSHIP, OVERSIZED = "chip-filling-512", "flagship-N256", "oversized-N1024"
FLEET_NAMES = RANDOM_NAMES + (CHIP_FILLING, FLAGSHIP, OVERSIZED) + TIE_NAMES


def build_fleets():
    """Every fleet, built once (module-scoped fixture in the tests); prints
    the build time, the redraws with their reasons and the coverage, and
    asserts the redraw cap and the coverage floor."""
    started = time.perf_counter()
    fleets = [random_fleet(seed, i) for i, seed in enumerate(RANDOM_SEEDS)]
    fleets += [chip_filling_fleet(), flagship_chain_fleet(), oversized_fleet()]
    fleets += [build_tie_fleet(i) for i in range(len(TIES))]
    elapsed = time.perf_counter() - started
    assert tuple(f.name for f in fleets) == FLEET_NAMES

    drawn = sum(f.drawn for f in fleets)
    reasons = Counter()
    for f in fleets:
        reasons.update(f.redrawn)
    redrawn = sum(reasons.values())
    pairs = sum(len(ps) for f in fleets for ps in f.pairs.values())
    print(
        f"fleet oracle: {len(fleets)} fleets, {drawn - redrawn} servers, {pairs} pairs "
        f"({sum(f.rows() for f in fleets)} solved by the oracle) in {elapsed:.1f} s; "
        f"redrawn {redrawn} of {drawn} servers: {dict(reasons)}"
    )
    assert redrawn <= MAX_DROP_SHARE * drawn, f"{redrawn} of {drawn} servers redrawn"

    counts = coverage_of(fleets)
    print(f"fleet oracle coverage: {counts}")
    for what, floor in MIN_COVERAGE.items():
        assert counts.get(what, 0) >= floor, f"only {counts.get(what, 0)} pairs {what}"
    assert counts["target subsets"] == 8  # every subset of ttft/itl/tps equal to 0
    rnd = fleets[: len(RANDOM_SEEDS)]
    assert {len(f.spec.servers.spec) for f in rnd} >= {1, 12}
    assert {len(f.spec.accelerators.spec) for f in rnd} == {3, 4}
    assert any(f.energy for f in rnd) and any(f.headroom for f in rnd)
    assert all(p.batch_size <= ORACLE_MAX_N for f in rnd for p in f.solved_pairs())
    return fleets


def fresh_spec(fleet: Fleet) -> SystemSpec:
    """A private copy: servers write their desired allocation into the spec."""
    return copy.deepcopy(fleet.spec)
