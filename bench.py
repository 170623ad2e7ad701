"""Flagship benchmark: global autoscaling solve on a synthetic MI355X fleet.

Measures the BASELINE.json headline metric — solver wall-clock (ms) with
SLO-attainment (%) — for N models x M accelerator types (config #3: 3
models x 2 service classes on 8xMI355X nodes, heterogeneous pool of 3
accelerator types).  One *step* is one full optimization cycle exactly as
the reconciler runs it: build the System from the cycle's observed loads,
size every (server, accelerator) pair (the analytic hot loop, batched on
the GPU via the gfx950 queue-solver kernel when available), run the
global min-cost solve, aggregate by type and export the solution.

The headline solve is CAPACITY-CONSTRAINED: the
fleet runs against a finite pool of 8-GPU MI355X nodes plus the
heterogeneous emulated parts, so the greedy limited-mode path — regret
ordering, binary-search reinsertion, saturation policy
(/root/reference/pkg/solver/greedy.go:35-104) — is what is timed, and
SLO attainment is a real solver-quality figure (unallocated or
over-target variants count as misses), not an identity.  The easier
unlimited argmin solve (the reference's hardwired production path) is
timed as a secondary series and reported in the same JSON line.

Scaling is WEAK: each rank owns a fixed shard of VARIANTS_PER_GPU variants
(a fleet shard), so N GPUs optimize an N-times-larger fleet; the reported
per-step wall-clock is the max over ranks after a barrier, i.e. the time
for the WHOLE fleet's global solve.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
(launched by torchrun for N>1; reads RANK/WORLD_SIZE/MASTER_* from env).

A plain run does only what the headline needs: warm up, time the K
capacity-constrained steps, print the result line.  ``--full`` adds the
secondary measurements (the unlimited-solve series and the closed-loop
observed-SLO run) to the same line.  ``--dump-outputs DIR`` writes what
the last timed step computed (``solution.npy``, ``sizing.npy``; see
``dump_outputs``) so two builds can be compared output for output.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import numpy as np
import torch

from wva_amd.config import (
    AcceleratorData,
    AllocationData,
    CapacityData,
    ModelData,
    OptimizerData,
    OptimizerSpec,
    ServerData,
    ServerLoadSpec,
    ServerSpec,
    ServiceClassData,
    ServiceClassSpec,
    ModelTarget,
    SystemSpec,
)
from wva_amd.config.mi355x import MI355X_CATALOG
from wva_amd.config.types import DecodeParmsSpec, ModelAcceleratorPerfData, PrefillParmsSpec
from wva_amd.core import System
from wva_amd.solver import Manager, Optimizer

VARIANTS_PER_GPU = 64  # fleet shard per rank (weak scaling)
MODELS = ["llama-8b", "llama-70b", "mixtral-8x7b"]
CLASSES = [("Premium", 1), ("Freemium", 10)]
ACCELERATORS = list(MI355X_CATALOG)  # MI355X, MI300X, L40S

# per-(model, accelerator) linear perf profiles (random-init per BASELINE:
# deterministic seeded values of realistic magnitude; no network for real
# fitted profiles)
_PROFILE_RNG = np.random.default_rng(42)
PROFILES = {}
for model_name in MODELS:
    scale = {"llama-8b": 1.0, "llama-70b": 3.0, "mixtral-8x7b": 2.0}[model_name]
    for acc_i, acc in enumerate(ACCELERATORS):
        slow = {"MI355X": 1.0, "MI300X": 1.6, "L40S": 6.0}[acc]
        PROFILES[(model_name, acc)] = dict(
            alpha=float(3.0 * scale * slow * _PROFILE_RNG.uniform(0.9, 1.1)),
            beta=float(0.03 * scale * slow * _PROFILE_RNG.uniform(0.9, 1.1)),
            gamma=float(8.0 * scale * slow * _PROFILE_RNG.uniform(0.9, 1.1)),
            delta=float(0.0004 * scale * slow * _PROFILE_RNG.uniform(0.9, 1.1)),
            acc_count={"llama-8b": 1, "llama-70b": 4, "mixtral-8x7b": 2}[model_name],
        )

SLOS = {
    ("Premium", "llama-8b"): (20.0, 800.0),
    ("Premium", "llama-70b"): (40.0, 2000.0),
    ("Premium", "mixtral-8x7b"): (30.0, 1500.0),
    ("Freemium", "llama-8b"): (60.0, 4000.0),
    ("Freemium", "llama-70b"): (120.0, 8000.0),
    ("Freemium", "mixtral-8x7b"): (90.0, 6000.0),
}


def capacity_pool(n_variants: int) -> CapacityData:
    """Finite accelerator pool for this rank's fleet shard, in whole
    8-GPU MI355X nodes (config #3's node granularity) plus smaller
    heterogeneous pools.

    Calibration: the synthetic loads' unconstrained demand averages ~45
    MI355X per variant (measured via the unlimited solve); the pool is
    sized to ~85% of that, so every step faces genuine scarcity — the
    greedy path must rank by priority/regret and some variants spill to
    slower parts or go unallocated, making SLO attainment a real solver
    -quality figure."""
    from wva_amd.config.types import AcceleratorCount

    mi355_nodes = max(1, (n_variants * 38 + 7) // 8)  # ~85% of demand
    return CapacityData(
        count=[
            AcceleratorCount(type="AMD-MI355X-288GB", count=8 * mi355_nodes),
            AcceleratorCount(type="AMD-MI300X-192GB", count=8 * n_variants),
            AcceleratorCount(type="EMU-L40S-48GB", count=8 * n_variants),
        ]
    )


def build_system_spec(
    rank: int, step: int, n_variants: int, limited: bool = True
) -> SystemSpec:
    """Synthetic cluster state for this rank at this step (loads vary per
    step so every cycle is a fresh solve)."""
    rng = np.random.default_rng(10_000 * (rank + 1) + step)
    replicas = rng.integers(1, 8, n_variants)
    rates = rng.uniform(30.0, 36000.0, n_variants)  # req/min
    in_tokens = rng.integers(64, 2048, n_variants)
    out_tokens = rng.integers(32, 1024, n_variants)
    servers = []
    for i in range(n_variants):
        model = MODELS[i % len(MODELS)]
        cls = CLASSES[(i // len(MODELS)) % len(CLASSES)][0]
        servers.append(
            ServerSpec(
                name=f"va-{rank}-{i}:bench",
                class_name=cls,
                model=model,
                keep_accelerator=False,
                min_num_replicas=1,
                max_batch_size=256,
                current_alloc=AllocationData(
                    accelerator="MI355X",
                    num_replicas=int(replicas[i]),
                    load=ServerLoadSpec(
                        arrival_rate=float(rates[i]),
                        avg_in_tokens=int(in_tokens[i]),
                        avg_out_tokens=int(out_tokens[i]),
                    ),
                ),
            )
        )
    return SystemSpec(
        accelerators=AcceleratorData(spec=list(MI355X_CATALOG.values())),
        models=ModelData(
            perf_data=[
                ModelAcceleratorPerfData(
                    name=m,
                    acc=a,
                    acc_count=PROFILES[(m, a)]["acc_count"],
                    max_batch_size=256,
                    decode_parms=DecodeParmsSpec(
                        alpha=PROFILES[(m, a)]["alpha"], beta=PROFILES[(m, a)]["beta"]
                    ),
                    prefill_parms=PrefillParmsSpec(
                        gamma=PROFILES[(m, a)]["gamma"], delta=PROFILES[(m, a)]["delta"]
                    ),
                )
                for m in MODELS
                for a in ACCELERATORS
            ]
        ),
        service_classes=ServiceClassData(
            spec=[
                ServiceClassSpec(
                    name=cls,
                    priority=prio,
                    model_targets=[
                        ModelTarget(
                            model=m, slo_itl=SLOS[(cls, m)][0], slo_ttft=SLOS[(cls, m)][1]
                        )
                        for m in MODELS
                    ],
                )
                for cls, prio in CLASSES
            ]
        ),
        servers=ServerData(spec=servers),
        optimizer=OptimizerData(
            spec=OptimizerSpec(
                unlimited=not limited,
                saturation_policy="PriorityRoundRobin" if limited else "",
            )
        ),
        capacity=capacity_pool(n_variants) if limited else CapacityData(),
    )


def one_cycle(
    rank: int, step: int, n_variants: int, device, limited: bool = True,
    keep_system: bool = False,
) -> dict:
    """One full optimization cycle; returns solution stats (plus the solved
    System under "system" when ``keep_system``)."""
    from wva_amd.ops import BatchedAllocationSolver

    spec = build_system_spec(rank, step, n_variants, limited=limited)
    system = System()
    optimizer_spec = system.set_from_spec(spec)
    BatchedAllocationSolver(device=device).calculate(system)
    manager = Manager(system, Optimizer(optimizer_spec))
    manager.optimize()
    solution = system.generate_solution()

    # SLO attainment: fraction of variants whose chosen allocation meets
    # the class targets and is not saturated at the offered load
    met, total = 0, 0
    for name, server in system.servers.items():
        total += 1
        alloc = server.allocation
        if alloc is None or alloc.num_replicas == 0:
            continue
        target = system.service_class(server.service_class_name).model_target(server.model_name)
        if (
            (target.itl == 0 or alloc.itl <= target.itl * 1.001)
            and (target.ttft == 0 or alloc.ttft <= target.ttft * 1.001)
            and not server.saturated()
        ):
            met += 1
    stats = {"solved": len(solution.spec), "slo_met": met, "total": total}
    if keep_system:
        stats["system"] = system
    return stats


# columns of the dumped arrays (accelerator = index into ACCELERATORS)
SOLUTION_COLUMNS = ("accelerator", "num_replicas", "max_batch", "cost",
                    "itl_average", "ttft_average")
SIZING_COLUMNS = ("num_replicas", "batch_size", "cost", "itl", "ttft", "rho",
                  "max_arrv_rate_per_replica")


def dump_outputs(system: System, out_dir: str, suffix: str = "") -> None:
    """Write what one cycle computed as float64 ``.npy`` files.

    - ``solution.npy`` [variants, len(SOLUTION_COLUMNS)]: the exported
      allocation solution, one row per variant in spec order; a variant
      left unallocated is accelerator -1 and zeros.
    - ``sizing.npy`` [variants, accelerators, len(SIZING_COLUMNS)]: the
      batched sizing result for every (variant, accelerator) pair; an
      infeasible pair is a row of zeros.
    """
    os.makedirs(out_dir, exist_ok=True)
    acc_index = {a: i for i, a in enumerate(ACCELERATORS)}
    solved = system.allocation_solution.spec
    n = len(system.servers)
    solution = np.zeros((n, len(SOLUTION_COLUMNS)), dtype=np.float64)
    sizing = np.zeros((n, len(ACCELERATORS), len(SIZING_COLUMNS)), dtype=np.float64)
    for i, (name, server) in enumerate(system.servers.items()):
        data = solved.get(name)
        if data is None:
            solution[i, 0] = -1.0
        else:
            solution[i] = (
                acc_index[data.accelerator], data.num_replicas, data.max_batch,
                data.cost, data.itl_average, data.ttft_average,
            )
        for acc, alloc in server.all_allocations.items():
            sizing[i, acc_index[acc]] = (
                alloc.num_replicas, alloc.batch_size, alloc.cost, alloc.itl,
                alloc.ttft, alloc.rho, alloc.max_arrv_rate_per_replica,
            )
    np.save(os.path.join(out_dir, f"solution{suffix}.npy"), solution)
    np.save(os.path.join(out_dir, f"sizing{suffix}.npy"), sizing)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variants-per-gpu", type=int, default=VARIANTS_PER_GPU)
    ap.add_argument("--backend", default="", help="override torch.distributed backend (default: nccl on GPU, gloo on CPU)")
    ap.add_argument("--no-observed-slo", action="store_true",
                    help="with --full: skip the untimed closed-loop observed-SLO measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements: the unlimited-solve "
                    "series and the closed-loop observed-SLO run")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(world_size, args.gpus)

    has_gpu = torch.cuda.is_available()
    if has_gpu:
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
        device = "cuda"
    else:
        device = "cpu"

    dist = None
    if world_size > 1:
        import torch.distributed as dist_mod

        backend = args.backend or ("nccl" if has_gpu else "gloo")
        dist_mod.init_process_group(backend=backend)
        dist = dist_mod

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if has_gpu:
            torch.cuda.synchronize()

    n_variants = args.variants_per_gpu

    # warmup (untimed)
    for step in range(args.warmup):
        one_cycle(rank, step, n_variants, device, limited=True)
        if args.full:
            one_cycle(rank, step, n_variants, device, limited=False)

    # headline: capacity-constrained greedy solve
    barrier_sync()
    t0 = time.perf_counter()
    stats = []
    # only the last step's System is kept (and only for --dump-outputs),
    # so every other step frees its objects exactly as an undumped run
    keep_at = args.steps - 1 if args.dump_outputs else -1
    for step in range(args.steps):
        stats.append(
            one_cycle(rank, args.warmup + step, n_variants, device, limited=True,
                      keep_system=step == keep_at)
        )
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        dump_outputs(
            stats[-1].pop("system"), args.dump_outputs,
            suffix=f".rank{rank}" if world_size > 1 else "",
        )

    # secondary series: the unlimited argmin solve on the same cycles
    elapsed_unlimited = 0.0
    if args.full:
        barrier_sync()
        t0u = time.perf_counter()
        for step in range(args.steps):
            one_cycle(rank, args.warmup + step, n_variants, device, limited=False)
        barrier_sync()
        elapsed_unlimited = time.perf_counter() - t0u

    # max over ranks (collectives need device tensors under RCCL)
    if dist is not None:
        coll_device = "cuda" if (has_gpu and dist.get_backend() == "nccl") else "cpu"
        t = torch.tensor(
            [elapsed, elapsed_unlimited], dtype=torch.float64, device=coll_device
        )
        slo = torch.tensor(
            [sum(s["slo_met"] for s in stats), sum(s["total"] for s in stats)],
            dtype=torch.float64,
            device=coll_device,
        )
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(slo, op=dist.ReduceOp.SUM)
        elapsed, elapsed_unlimited = float(t[0].item()), float(t[1].item())
        slo_met, slo_total = float(slo[0].item()), float(slo[1].item())
    else:
        slo_met = float(sum(s["slo_met"] for s in stats))
        slo_total = float(sum(s["total"] for s in stats))

    ms_per_step = elapsed / args.steps * 1000.0
    secondary = {}
    if args.full:
        secondary["unlimited_ms_per_step"] = elapsed_unlimited / args.steps * 1000.0
    slo_attainment = 100.0 * slo_met / slo_total if slo_total else 0.0

    # Observed SLO attainment (untimed, single-rank runs only): a short
    # closed loop against the scalable emulator fleet — load -> scrape ->
    # solve -> resize -> measured TTFT/ITL vs targets (VERDICT r01 #2:
    # attainment measured from serving latency, not from the sizing
    # model's own predictions).
    observed = {}
    if args.full and rank == 0 and world_size == 1 and not args.no_observed_slo:
        sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
        sys.path.insert(0, str(Path(__file__).resolve().parent / "tests"))
        try:
            from soak import run_soak

            soak_result = run_soak(
                stages=(2.0, 4.0, 6.0, 4.0), stage_seconds=5.0,
                max_replicas=4, quiet=True,
            )
            observed = {
                "observed_slo_attainment_pct": soak_result[
                    "observed_slo_attainment_pct"
                ],
                "mean_itl_drift_pct": soak_result["mean_itl_drift_pct"],
            }
        except Exception as e:  # pragma: no cover - env-dependent
            observed = {"observed_slo_attainment_pct": None,
                        "observed_slo_error": str(e)[:200]}

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "solver_wall_clock_ms",
                    "value": ms_per_step,
                    "unit": "ms",
                    "n_gpus": n_gpus,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": False,
                    "scaling": "weak",
                    "vs_baseline": None,
                    "dtype": "fp64",
                    "data": "synthetic",
                    "slo_attainment_pct": slo_attainment,
                    **secondary,
                    **observed,
                    "config": {
                        "model": "3 models x 2 service classes (config #3)",
                        "variants": n_gpus * n_variants,
                        "accelerator_types": len(ACCELERATORS),
                        "sizing_problems_per_step": n_gpus * n_variants * len(ACCELERATORS),
                        "global_batch": n_gpus * n_variants,
                        "seq_len": 0,
                        "parallelism": f"fleet-shard dp{n_gpus}",
                        "analyzer_device": device,
                        "solver_mode": "greedy-limited (PriorityRoundRobin), "
                        "capacity: 8xMI355X nodes + heterogeneous pool",
                    },
                }
            )
        )

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
