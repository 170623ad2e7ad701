"""The sizing cycle of a fleet that needs the M/G/1 correction.

``BatchedAllocationSolver`` resolves every server's service-time cs^2 (its
measured ``service_scv``, or the fleet value for the -1 sentinel) and hands
the vector to the same native path that sizes a Markovian fleet.  This module
checks that hand-over on a 6-server x 3-accelerator fleet from
tests/fixtures.py whose ``service_scv`` values are drawn from
``{-1, 0, 0.4, 1.0, 2.0}``, under ``WVA_ANALYZER=mg1 WVA_SERVICE_SCV=0.5``
and with the environment unset (fleet value 1.0):

- the vector that reaches the solver equals the resolved cs^2 of each row's
  server, slice by slice;
- allocations are bit-equal across chunk counts on one device;
- against ``System.calculate()`` — the scalar analyzer — under the same
  environment: the same candidates in the same order, replicas, batch size
  and cost bit-equal, ITL, TTFT, rho and the per-replica rate within twice the
  row's ``row_bound`` (test_ops_oracle_wide.py), because both sides are within
  one bound of the oracle;
- the Python analyzer is not called when a native binding is built, and on
  the GPU the plan is the asynchronous native dispatch.

The fleet is checked at construction to put no replica quotient within 1e-6
of an integer, so that ``ceil`` cannot legitimately differ between two
correct solvers.
"""

from __future__ import annotations

import numpy as np
import pytest

import mm1k_oracle
import wva_amd.ops as ops
import wva_amd.ops.batched as B
from fixtures import make_spec, server_spec
from test_ops_oracle_wide import row_bound
from wva_amd.core import System
from wva_amd.ops import BatchedAllocationSolver, native_available, native_cpu_available

SEED = 20250214
SCV_VALUES = (-1.0, 0.0, 0.4, 1.0, 2.0)
CHUNKS = (1, 2, 3)
ENVS = {
    "mg1": {"WVA_ANALYZER": "mg1", "WVA_SERVICE_SCV": "0.5"},
    "unset": {},
}
FLEET_SCV = {"mg1": 0.5, "unset": 1.0}
QUOTIENT_MARGIN = 1e-6

ALLOCATION_FIELDS = (
    "accelerator", "num_replicas", "batch_size", "cost", "value", "itl", "ttft",
    "rho", "max_arrv_rate_per_replica",
)


def _servers():
    # a and b are loaded so that the correction moves a replica count: on
    # MI300X the Markovian quotients are 2.015 and 3.97, and the cs^2 drawn
    # for them (0 and 2) scale the per-replica rate by 1.033 and 0.986
    servers = [
        server_spec("a:ns", arrival_rate=915.0),
        server_spec("b:ns", model="llama-70b", arrival_rate=1575.0, max_batch=16),
        server_spec("c:ns", class_name="Freemium", arrival_rate=90.0, in_tokens=700,
                    out_tokens=333, cur_accelerator="MI300X", cur_replicas=3),
        server_spec("d:ns", arrival_rate=4800.0, max_batch=64, min_replicas=2),
        server_spec("e:ns", model="llama-70b", class_name="Freemium", arrival_rate=30.0,
                    max_batch=0),  # N from the perf data
        server_spec("f:ns", arrival_rate=2400.0, in_tokens=1024, out_tokens=64, max_batch=32),
    ]
    # every value once, in a drawn order, and one more draw for the sixth
    rng = np.random.default_rng(SEED)
    drawn = list(rng.permutation(SCV_VALUES)) + [rng.choice(SCV_VALUES)]
    assert set(drawn) == set(SCV_VALUES)
    for server, scv in zip(servers, drawn):
        server.service_scv = float(scv)
    return servers


def new_system():
    system = System()
    system.set_from_spec(make_spec(servers=_servers()))
    assert len(system.servers) == 6 and len(system.accelerators) == 3
    return system


def rows_per_server():
    """How many sizing rows each server contributes: one per accelerator its
    model has a profile on (the fixture has no llama-70b profile on L40S)."""
    spec = make_spec(servers=_servers())
    profiled = {(p.name, p.acc) for p in spec.models.perf_data}
    accs = [a.name for a in spec.accelerators.spec]
    return [(s, sum((s.model, acc) in profiled for acc in accs)) for s in spec.servers.spec]


def expected_vector(env):
    out = []
    for server, n_rows in rows_per_server():
        scv = server.service_scv if server.service_scv >= 0 else FLEET_SCV[env]
        out += [scv] * n_rows
    assert len(out) == 16 and len(set(out)) >= 4
    return np.array(out, dtype=np.float64)


def fields_of(alloc):
    return tuple(getattr(alloc, f) for f in ALLOCATION_FIELDS)


def snapshot(system):
    return {name: [(acc, fields_of(a)) for acc, a in s.all_allocations.items()]
            for name, s in system.servers.items()}


def set_env(mp, env):
    mp.delenv("WVA_ANALYZER", raising=False)
    mp.delenv("WVA_SERVICE_SCV", raising=False)
    mp.delenv("WVA_SIZING_HEADROOM", raising=False)
    mp.delenv("WVA_GPU_GRAPH", raising=False)
    for key, value in ENVS[env].items():
        mp.setenv(key, value)


def sized(env, device, chunks):
    """A fresh system sized by the batched solver.  Returns the system, the
    problem slices handed to the dispatch, and the cs^2 vector that reached
    the solver with each: ``solve_problems`` on the CPU, the native
    ``submit`` on the GPU."""
    system = new_system()
    slices, vectors = [], []
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, env)
        for dispatch in (B.SyncDispatch, B.NativeGpuDispatch):
            def submit(self, problems, scv_rows=None, _real=dispatch.submit):
                slices.append(np.array(problems, dtype=np.float64, copy=True))
                return _real(self, problems, scv_rows)

            mp.setattr(dispatch, "submit", submit)

        def keep(scv):
            vectors.append(None if scv is None else np.array(scv, copy=True))

        if device == "cpu":
            real_solve = B.solve_problems

            def solve_spy(problems, device=None, scv=None):
                keep(scv)
                return real_solve(problems, device, scv=scv)

            mp.setattr(B, "solve_problems", solve_spy)
        else:
            native = ops.get_native()
            real_submit = native.submit

            def submit_spy(problems, max_k, scv=None):
                keep(scv)
                return real_submit(problems, max_k, scv)

            mp.setattr(native, "submit", submit_spy)
        if native_cpu_available() or native_available():
            def analyzer_used(*args, **kwargs):
                raise AssertionError("the Python analyzer was used although a native "
                                     "binding is built")

            mp.setattr(B, "_solve_problems_python", analyzer_used)
        BatchedAllocationSolver(device=device, chunks=chunks).calculate(system)
    return system, slices, vectors


@pytest.fixture(scope="module")
def reference():
    """Per environment: ``System.calculate()`` (the scalar analyzer), sized
    once and left alone, and the fleet's problem rows in order."""
    out = {}
    for env in ENVS:
        with pytest.MonkeyPatch.context() as mp:
            set_env(mp, env)
            system = new_system()
            system.calculate()
        _, slices, _ = sized(env, "cpu", 1)
        rows = np.concatenate(slices)
        assert rows.shape == (16, 12)
        out[env] = (system, rows)
    return out


def row_index():
    """(server name, accelerator) of every problem row, in order."""
    spec = make_spec(servers=_servers())
    profiled = {(p.name, p.acc) for p in spec.models.perf_data}
    return [(s.name, a.name) for s in spec.servers.spec for a in spec.accelerators.spec
            if (s.model, a.name) in profiled]


def test_fleet_is_clear_of_integer_quotients_and_feels_the_correction(reference):
    """Construction checks, on the CPU: no replica quotient within 1e-6 of an
    integer, and the correction really moves this fleet's answers."""
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, "unset")
        markovian = System()
        spec = make_spec(servers=_servers())
        for s in spec.servers.spec:
            s.service_scv = -1.0
        markovian.set_from_spec(spec)
        markovian.calculate()
    for env, (system, rows) in reference.items():
        sized_pairs = 0
        for (name, acc), row in zip(row_index(), rows):
            alloc = system.servers[name].all_allocations.get(acc)
            if alloc is None:
                continue
            sized_pairs += 1
            quotient = row[B.P_TOTAL_RATE] / (alloc.max_arrv_rate_per_replica * 1000.0)
            nearest = round(quotient)
            assert nearest < 1 or abs(quotient - nearest) > QUOTIENT_MARGIN * nearest, (
                env, name, acc, quotient)
        assert sized_pairs >= 12
        moved = [
            (name, acc)
            for name, server in system.servers.items()
            for acc, a in server.all_allocations.items()
            if a.num_replicas != markovian.servers[name].all_allocations[acc].num_replicas
        ]
        print(f"{env}: replica count differs from the Markovian fleet's on {moved}")
        assert moved, f"{env}: the correction changes no replica count of this fleet"


def check_vectors(env, slices, vectors):
    want = expected_vector(env)
    assert len(vectors) == len(slices) >= 1
    offset = 0
    for rows, vector in zip(slices, vectors):
        assert vector is not None and vector.dtype == np.float64
        np.testing.assert_array_equal(vector, want[offset:offset + len(rows)])
        offset += len(rows)
    assert offset == len(want)


def check_against_scalar(env, system, reference, label):
    ref_system, rows = reference[env]
    by_pair = dict(zip(row_index(), rows))
    for name, server in system.servers.items():
        ref = ref_system.servers[name].all_allocations
        assert list(server.all_allocations) == list(ref), f"{label} {name}: candidates"
        for acc, a in server.all_allocations.items():
            r, tag = ref[acc], f"{label} {name}/{acc}"
            assert (a.accelerator, a.num_replicas, a.batch_size, a.cost) == (
                r.accelerator, r.num_replicas, r.batch_size, r.cost), tag
            row = by_pair[(name, acc)]
            rate = row[B.P_TOTAL_RATE] / r.num_replicas / 1000.0  # req/ms per replica
            scale = max(mm1k_oracle.log_table_scale(row, r.max_arrv_rate_per_replica),
                        mm1k_oracle.log_table_scale(row, rate))
            bound = 2 * row_bound(scale)
            # the oracle tests' error measures: relative, TTFT against the
            # response time (serv = n_serv / throughput = rho * N / rate)
            serv = r.rho * r.batch_size / rate
            errs = {
                "itl": abs(a.itl - r.itl) / r.itl,
                "rho": abs(a.rho - r.rho) / r.rho,
                "rate": abs(a.max_arrv_rate_per_replica / r.max_arrv_rate_per_replica - 1.0),
                "ttft": abs(a.ttft - r.ttft) / (r.ttft + serv),
            }
            for what, err in errs.items():
                assert err <= bound, f"{tag}: {what} off by {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("env", list(ENVS))
def test_batched_cpu(env, reference):
    snapshots = []
    for chunks in CHUNKS:
        system, slices, vectors = sized(env, "cpu", chunks)
        check_vectors(env, slices, vectors)
        check_against_scalar(env, system, reference, f"cpu {env} chunks={chunks}")
        snapshots.append(snapshot(system))
    assert snapshots[1] == snapshots[0] and snapshots[2] == snapshots[0]


@pytest.mark.parametrize("env", list(ENVS))
def test_plan_off_the_gpu_is_one_synchronous_chunk(env):
    with pytest.MonkeyPatch.context() as mp:
        set_env(mp, env)
        system = new_system()
        dispatch, n_chunks, track = BatchedAllocationSolver(device="cpu", chunks=3)._plan(
            system, list(system.servers.values()))
    assert isinstance(dispatch, B.SyncDispatch) and n_chunks == 1 and track
    assert dispatch.global_scv == FLEET_SCV[env]


@pytest.mark.gpu
class TestGPUCycleMG1:
    @pytest.fixture(autouse=True)
    def _pool_is_idle_afterwards(self):
        yield
        assert ops.get_native().dispatch_pool_stats()[1] == 0

    @pytest.mark.parametrize("env", list(ENVS))
    def test_plan_is_the_native_dispatch(self, env):
        with pytest.MonkeyPatch.context() as mp:
            set_env(mp, env)
            system = new_system()
            dispatch, n_chunks, track = BatchedAllocationSolver(device="cuda")._plan(
                system, list(system.servers.values()))
        assert isinstance(dispatch, B.NativeGpuDispatch) and track
        assert n_chunks == B.DEFAULT_GPU_CHUNKS  # the Markovian chunk rule
        assert dispatch.global_scv == FLEET_SCV[env]

    @pytest.mark.parametrize("env", list(ENVS))
    def test_batched_gpu(self, env, reference):
        snapshots = []
        for chunks in CHUNKS:
            system, slices, vectors = sized(env, "cuda", chunks)
            assert len(slices) == chunks
            check_vectors(env, slices, vectors)
            check_against_scalar(env, system, reference, f"gpu {env} chunks={chunks}")
            snapshots.append(snapshot(system))
        assert snapshots[1] == snapshots[0] and snapshots[2] == snapshots[0]
