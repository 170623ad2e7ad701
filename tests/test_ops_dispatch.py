"""The native asynchronous sizing dispatch (submit/collect) on the GPU.

submit/collect must return bit for bit what the tensor API
(``solve_allocations``) returns for the same rows and the same ``max_k``:
both go through the same launcher, so the same kernel geometry runs.
"""

import threading

import numpy as np
import pytest

from wva_amd.ops import BatchedAllocationSolver
from wva_amd.ops.batched import MAX_QUEUE_TO_BATCH_RATIO, PROBLEM_FIELDS, R_FEASIBLE

from fixtures import make_system, server_spec

pytestmark = pytest.mark.gpu

CHAIN = 1 + MAX_QUEUE_TO_BATCH_RATIO


def problems_for(b, n, seed):
    """b feasible-leaning rows with batch limit n."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(2.0, 25.0, b)
    beta = rng.uniform(0.005, 0.5, b)
    gamma = rng.uniform(2.0, 60.0, b)
    delta = rng.uniform(0.001, 0.2, b)
    in_tok = rng.integers(0, 2048, b).astype(np.float64)
    out_tok = rng.integers(1, 1024, b).astype(np.float64)
    t_itl = alpha + beta * 2 + rng.uniform(1.0, 30.0, b)
    t_ttft = gamma + delta * in_tok * 2 + rng.uniform(10.0, 5000.0, b)
    t_tps = np.where(rng.random(b) < 0.7, 0.0, rng.uniform(100.0, 5000.0, b))
    rate = rng.uniform(0.01, 500.0, b)
    min_rep = rng.integers(0, 3, b).astype(np.float64)
    return np.ascontiguousarray(np.stack(
        [alpha, beta, gamma, delta, in_tok, out_tok, np.full(b, float(n)),
         t_ttft, t_itl, t_tps, rate, min_rep], axis=1))


@pytest.fixture(scope="module")
def native():
    from wva_amd.ops import get_native

    mod = get_native()
    assert mod is not None and mod.HAS_HIP
    return mod


def tensor_api(native, problems, max_k):
    import torch

    return native.solve_allocations(torch.from_numpy(problems).cuda(), max_k).cpu().numpy()


@pytest.mark.parametrize("n", [1, 8, 64])
@pytest.mark.parametrize("b", [1, 5, 192])
def test_bit_equal_to_tensor_api(native, b, n):
    problems = problems_for(b, n, seed=100 * b + n)
    got = native.collect(native.submit(problems, n * CHAIN))
    assert got.dtype == np.float64 and got.shape == (b, 6)
    np.testing.assert_array_equal(got, tensor_api(native, problems, n * CHAIN))
    if b > 1:
        assert got[:, R_FEASIBLE].sum() > 0


def test_three_in_flight_collected_in_reverse(native):
    batches = [problems_for(b, n, seed=7 + b) for b, n in ((192, 64), (5, 8), (1, 1))]
    max_ks = [64 * CHAIN, 8 * CHAIN, CHAIN]
    tickets = [native.submit(p, k) for p, k in zip(batches, max_ks)]
    assert len(set(tickets)) == 3
    slots, busy = native.dispatch_pool_stats()
    assert busy == 3 and slots >= 3
    for ticket, p, k in reversed(list(zip(tickets, batches, max_ks))):
        np.testing.assert_array_equal(native.collect(ticket), tensor_api(native, p, k))
    assert native.dispatch_pool_stats()[1] == 0


def test_buffers_grow_and_shrink_back(native):
    # 5 rows, then more than any slot holds so far, then 5 again
    for b in (5, 300, 5):
        problems = problems_for(b, 8, seed=b)
        got = native.collect(native.submit(problems, 8 * CHAIN))
        np.testing.assert_array_equal(got, tensor_api(native, problems, 8 * CHAIN))


def test_rows_outside_the_contract_are_zero_rows(native):
    problems = problems_for(8, 8, seed=3)
    good = problems.copy()
    problems[1, 0] = np.nan          # non-finite field
    problems[2, 0] = -1.0            # negative alpha
    problems[3, 6] = 0.0             # N < 1
    problems[4, 5] = 0.0             # no output tokens
    problems[5, 8] = -5.0            # negative target
    problems[6, 6] = 64.0            # chain longer than this launch reserved
    got = native.collect(native.submit(problems, 8 * CHAIN))
    want = native.collect(native.submit(good, 8 * CHAIN))
    assert (got[1:7] == 0.0).all()
    np.testing.assert_array_equal(got[[0, 7]], want[[0, 7]])
    assert want[[0, 7], R_FEASIBLE].sum() > 0


def test_empty_batch_is_an_empty_result(native):
    # B = 0 has nothing to solve: a ticket, an empty [0, 6] result, no slot
    before = native.dispatch_pool_stats()
    ticket = native.submit(np.zeros((0, PROBLEM_FIELDS)), CHAIN)
    assert native.dispatch_pool_stats() == before
    out = native.collect(ticket)
    assert out.shape == (0, 6) and out.dtype == np.float64
    with pytest.raises(ValueError, match="already collected"):
        native.collect(ticket)


def test_bad_tickets_and_arguments_raise(native):
    with pytest.raises(ValueError, match="unknown sizing ticket"):
        native.collect(1 << 40)
    with pytest.raises(ValueError, match="unknown sizing ticket"):
        native.collect(-3)
    problems = problems_for(5, 8, seed=1)
    ticket = native.submit(problems, 8 * CHAIN)
    native.collect(ticket)
    with pytest.raises(ValueError, match="already collected"):
        native.collect(ticket)
    with pytest.raises(TypeError):
        native.submit(problems.astype(np.float32), 8 * CHAIN)
    with pytest.raises(ValueError):
        native.submit(problems[:, :11].copy(), 8 * CHAIN)
    with pytest.raises(ValueError):
        native.submit(np.asfortranarray(problems), 8 * CHAIN)
    with pytest.raises(ValueError):
        native.submit(problems[0], 8 * CHAIN)
    assert native.dispatch_pool_stats()[1] == 0


def test_lds_refusal_raises_and_leaves_the_pool_usable(native):
    problems = problems_for(5, 8, seed=2)
    # 9000 doubles of chain do not fit 64 KiB of LDS in any geometry: the
    # launcher refuses before launching anything
    with pytest.raises(RuntimeError, match="LDS"):
        native.submit(problems, 9000)
    assert native.dispatch_pool_stats()[1] == 0
    got = native.collect(native.submit(problems, 8 * CHAIN))
    np.testing.assert_array_equal(got, tensor_api(native, problems, 8 * CHAIN))


def test_two_threads_agree_with_serial(native):
    batches = [problems_for(5 + 3 * (i % 4), 8, seed=50 + i) for i in range(20)]
    serial = [native.collect(native.submit(p, 8 * CHAIN)) for p in batches]
    results = {}

    def worker(tag):
        results[tag] = [native.collect(native.submit(p, 8 * CHAIN)) for p in batches]

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for tag in range(2):
        assert len(results[tag]) == 20
        for got, want in zip(results[tag], serial):
            np.testing.assert_array_equal(got, want)
    assert native.dispatch_pool_stats()[1] == 0


def test_calculate_chunked_matches_single_launch():
    servers = [
        server_spec(f"s{i}:ns", arrival_rate=60.0 * (i + 1), in_tokens=100 + 37 * i,
                    out_tokens=64 + 11 * i, max_batch=(1, 8, 64)[i % 3],
                    model="llama-70b" if i % 4 == 3 else "llama-8b")
        for i in range(8)
    ]

    def solved(chunks):
        system, _ = make_system(servers=servers)
        BatchedAllocationSolver(device="cuda", chunks=chunks).calculate(system)
        return {
            name: [(acc, a.num_replicas, a.batch_size, a.cost, a.value, a.itl, a.ttft,
                    a.rho, a.max_arrv_rate_per_replica)
                   for acc, a in s.all_allocations.items()]
            for name, s in system.servers.items()
        }

    one = solved(1)
    assert sum(len(v) for v in one.values()) >= 8
    assert solved(3) == one
