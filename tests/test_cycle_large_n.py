"""The sizing cycle with a max-batch-1024 server kept on the GPU (``large_n``).

tests/fleet_oracle.py's ``oversized-N1024`` fleet has one server whose three
candidate rows have N = 1024.  Without the opt-in its chunk takes the
synchronous CPU split (test_cycle_oracle.py pins that); with it the chunk
stays on the asynchronous submit/collect dispatch: the rows within the old
limit in one launch, the N = 1024 rows in a compact-table launch next to it.
Every server is held to the checks test_cycle_oracle.py applies (order,
feasible set, the oracle's tolerances, bit-equal batch size, cost and value,
the optimizer's exported solutions), and the servers within the old limit must
not notice the opt-in at all.
"""

from __future__ import annotations

import numpy as np
import pytest

import fleet_oracle as fo
import wva_amd.ops as ops
import wva_amd.ops.batched as B
from test_cycle_oracle import check_fleet, fields_of, new_system, sized, sizing_env, solutions_of
from wva_amd.ops import BatchedAllocationSolver

CHUNKS = (1, 2, 3)


@pytest.fixture(scope="module")
def fleet():
    return fo.oversized_fleet()


@pytest.fixture(scope="module")
def scalar(fleet):
    system = sized(fleet, "scalar")
    return {fleet.name: (system, solutions_of(fleet, system))}


def sized_on_gpu(fleet, chunks, large_n, mp_extra=None):
    """As test_cycle_oracle.sized, with the opt-in; also returns the sizes of
    the launches by binding entry point and of any ``solve_problems`` call."""
    system = new_system(fleet)
    seen = {"submit": [], "submit_compact": [], "solve_problems": []}
    native = ops.get_native()
    with sizing_env(fleet, "gpu") as mp:
        if mp_extra is not None:
            mp_extra(mp)
        submitted = []

        # the opt-in's dispatch class forwards ordinary chunks to its parent
        # class: record a chunk once, at the class the solver picked
        def submit(self, problems, scv_rows=None):
            if getattr(self, "_recording", False):  # forwarded by the subclass
                return real_submit[B.NativeGpuDispatch](self, problems, scv_rows)
            submitted.append(np.array(problems, dtype=np.float64, copy=True))
            self._recording = True
            try:
                return real_submit[type(self)](self, problems, scv_rows)
            finally:
                self._recording = False

        real_submit = {c: c.submit for c in (B.NativeGpuDispatch, B.LargeNGpuDispatch)}
        for c in real_submit:
            mp.setattr(c, "submit", submit)
        for name in ("submit", "submit_compact"):
            def spy(*args, _real=getattr(native, name), _name=name):
                seen[_name].append(len(args[0]))
                return _real(*args)

            mp.setattr(native, name, spy)

        def solve_spy(problems, *args, _real=B.solve_problems, **kwargs):
            seen["solve_problems"].append(len(problems))
            return _real(problems, *args, **kwargs)

        mp.setattr(B, "solve_problems", solve_spy)
        BatchedAllocationSolver(device="cuda", chunks=chunks, large_n=large_n).calculate(system)
    system.submitted = np.concatenate(submitted)
    return system, seen


@pytest.mark.gpu
class TestGPUCycleLargeN:
    @pytest.fixture(autouse=True)
    def _pool_is_idle_afterwards(self, monkeypatch):
        monkeypatch.delenv("WVA_GPU_GRAPH", raising=False)
        monkeypatch.delenv("WVA_GPU_LARGE_N", raising=False)
        yield
        assert ops.get_native().dispatch_pool_stats()[1] == 0

    @pytest.mark.parametrize("chunks", CHUNKS)
    def test_oversized_server_stays_on_the_gpu(self, chunks, fleet, scalar):
        big_rows = sum(p.batch_size == fo.OVERSIZED_N for p in fleet.solved_pairs())
        assert big_rows == 3
        system, seen = sized_on_gpu(fleet, chunks, True)
        assert seen["solve_problems"] == [], "the synchronous split was taken"
        assert seen["submit_compact"] == [big_rows]  # one compact launch, in its chunk
        assert sum(seen["submit"]) == fleet.rows() - big_rows
        check_fleet(fleet, system, scalar, f"gpu large_n chunks={chunks}")

        # the servers within the old limit do not notice the opt-in
        plain, seen_off = sized_on_gpu(fleet, chunks, False)
        assert seen_off["submit_compact"] == [] and seen_off["solve_problems"]
        compared = 0
        for name, server in system.servers.items():
            pairs = [p for p in fleet.pairs[name] if p.kind == "solved"]
            if any(p.batch_size > B.GPU_MAX_BATCH_LIMIT for p in pairs):
                continue
            want = plain.servers[name].all_allocations
            assert list(server.all_allocations) == list(want)
            for acc, alloc in server.all_allocations.items():
                assert fields_of(alloc) == fields_of(want[acc]), f"{name}/{acc}"
                compared += 1
        assert compared >= 4

    def test_the_environment_takes_the_same_route(self, fleet, scalar):
        system, seen = sized_on_gpu(
            fleet, 2, None, lambda mp: mp.setenv("WVA_GPU_LARGE_N", "1"))
        assert seen["solve_problems"] == [] and seen["submit_compact"] == [3]
        check_fleet(fleet, system, scalar, "gpu WVA_GPU_LARGE_N=1")

    def test_off_by_default(self, fleet, scalar):
        system, seen = sized_on_gpu(fleet, 2, None)
        assert seen["submit_compact"] == [] and seen["solve_problems"]
        check_fleet(fleet, system, scalar, "gpu default")
