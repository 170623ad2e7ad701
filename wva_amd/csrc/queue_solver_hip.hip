// gfx950 (CDNA4) batched allocation-sizing kernel.
//
// One workgroup per problem: the whole analytic pipeline of
// core.create_allocation (service-rate table, log-space product-form
// M/M/1/K probabilities, TTFT/ITL bisection, replica count, final
// per-replica analysis) runs in-workgroup:
//
//   - the cumulative log-service-rate table (K = 11*N doubles) lives in
//     LDS and is built with a chunked parallel scan — every later model
//     evaluation is LDS-bound, never HBM; consecutive lanes touch
//     consecutive doubles -> conflict-free ds_read_b64;
//   - a model evaluation sweeps only the <= N+1 pre-batch states (wave64
//     __shfl_down reductions, 2x-unrolled exp); the whole constant-rate
//     queue region [N+1, K] — 10/11 of the states — sums in CLOSED FORM
//     (geo_tail in queue_core.h, expm1-based geometric sums), which also
//     made the 1e-16 significance window obsolete;
//   - the normalization mode comes from a wave-parallel 64-probe ballot
//     search (wave_lower_bound) instead of a serial bisection;
//   - the default spec geometry (384 = 2 search groups x 3 wave64) runs
//     the TTFT and ITL bisections concurrently AND speculatively: each
//     round a group evaluates its bracket's full depth-2 midpoint tree
//     (the midpoints are bitwise the sequential iterates) and consumes
//     two bisection levels; wave sync is group-local LDS mailboxes with a
//     watchdog — no workgroup barriers after the scan;
//   - every body starts the same way: threads 0..5 zero the result row,
//     then the row guard (row_rejected) ends the workgroup for a row that
//     breaks the contract of queue_core.h, or whose table exceeds what this
//     launch reserved, before LDS is touched; the same six threads write a
//     feasible row's values at the end;
//   - the solve itself is queue_core.h's (search_targets, row_tail), shared
//     with the host: a body only decides which threads evaluate what;
//   - a launch may carry one service-time cs^2 per row (M/G/1 correction,
//     queue_core.h): it scales the wait inside eval_ttft_of and nowhere
//     else, so every body and both searches pick it up through Parms;
//   - LDS budget: (max_k + THREADS + 64) doubles <= 64 KiB for N <= ~700;
//     the launcher checks it for the geometry it picked before launching
//     and the binding raises when it does not fit (batched.py routes
//     larger batch limits to the CPU path, or — opt-in — to the
//     compact-table kernel at the end of this file, which keeps N doubles
//     instead of 11*N and reaches N ~7800).
//
// Numerics are double throughout, matching the Python analyzer; parity
// is enforced by tests/test_ops.py, the @gpu numerics tests and
// tools/fuzz_parity.py (20k problems, zero feasibility flips).  Design
// narrative + measurements: docs/design/native-queue-solver.md,
// profiles/r02_kernel_notes.md.

#include <hip/hip_runtime.h>

#include "queue_core.h"

namespace wva {

// Five workgroup geometries are instantiated:
//   - 64 (sequential single wave, barrier-free __shfl reductions);
//   - 128 ("dual": wave 0 searches TTFT while wave 1 searches ITL —
//     the winner for chip-filling launches, B >= 512);
//   - 256 (4-wave strided sweeps + LDS cross-wave combine);
//   - 384 (speculative-tree multisection, depth 2 — the default for
//     underfilled, latency-bound launches);
//   - 896 (depth-3 speculation; measured slower than depth 2).
// The launcher auto-selects (occupancy-aware, see wva_launch_solve_scv);
// WVA_GPU_THREADS=64|128|256|384|896 overrides, read per launch.  A sixth
// kernel runs the 256 body over the compact table (N doubles, not 11*N).

// Reduction scratch layout (doubles, after cum[max_k] in dynamic LDS):
//   red[0..WAVES*5-1]  per-wave partials (S, Ni, Snum, Ninum, eK)

// Wave-parallel lower bound: smallest i in [lo, hi] with pred(i) true,
// for a monotone (false...false true...true) predicate with pred(hi)
// guaranteed true.  64 probes per round shrink the range 64x, replacing
// ~11 DEPENDENT binary-search iterations (each an LDS-latency chain)
// with ~2 ballot rounds of PARALLEL probes.  Exact: the boundary of a
// monotone predicate is unique, so any probe strategy lands on the same
// index the sequential bisection finds.
template <typename Pred>
__device__ inline int wave_lower_bound(int lo, int hi, int lane, Pred pred) {
  while (hi - lo >= 64) {
    const int step = (hi - lo + 63) >> 6;
    const int i = lo + lane * step;  // lane 0 probes lo itself
    const bool t = (i >= hi) ? true : pred(i);
    const unsigned long long mask = __ballot(t);
    if (mask == 0ull) {
      // every probe (all below hi) is false: boundary past the last one
      lo = lo + 63 * step + 1;
      continue;
    }
    const int first = __ffsll((long long)mask) - 1;
    if (first == 0) return lo;  // pred(lo) already true
    lo = lo + (first - 1) * step + 1;
    const int cap = lo - 1 + step;  // == previous lo + first*step
    if (cap < hi) hi = cap;
  }
  const int i = lo + lane;
  const bool t = (i >= hi) ? true : pred(i);
  const unsigned long long mask = __ballot(t);
  return lo + __ffsll((long long)mask) - 1;
}

// Table policies: what a workgroup keeps in LDS for its row.  A policy
// supplies the row guard's length test, the number of states build_cum
// scans, log_p(n), and the geometric tail with the sweep bound that goes
// with it.  Each takes the tail's d its own way (the difference of two table
// entries, or log(lam) - L_N directly) and has its own g_start / loop_hi
// rule; the two are not numerically interchangeable.

// cum[0..K-1], K = 11 * N; the launch reserves max_k doubles
struct LdsFullTable {
  const double *cum;
  int K;
  static __device__ bool fits(const double *pr, int max_k) {
    return row_chain_length(pr) <= max_k;
  }
  __device__ LdsFullTable(const Parms &p, const double *table)
      : cum(table), K(p.max_batch * (1 + kMaxQueueToBatchRatio)) {}
  __device__ int scan_length() const { return K; }
  __device__ int chain() const { return K; }
  __device__ double log_p(double loglam, int n) const { return wva::log_p(cum, loglam, n); }
  // closed-form sum of the states past N, up to 10/11 of the chain — the
  // per-state exp calls they would cost are the kernel's dominant fp64 work
  __device__ GeoTail tail(int num, double loglam, double m, int *loop_hi) const {
    const int g_start = num + 1;
    GeoTail t{0.0, 0.0, 0.0, false};
    *loop_hi = K;
    if (g_start + 8 <= K) {
      const double d = loglam - (cum[g_start] - cum[g_start - 1]);
      t = geo_tail(log_p(loglam, g_start) - m, d, g_start, K, K);
      if (t.used) *loop_hi = g_start - 1;
    }
    return t;
  }
};

// cum[0..N-1] only (queue_core.h, "Compact table"); the launch reserves
// max_n doubles.  The sweep over the N+1 pre-batch states reads cum[n-1]
// with n-1 <= N-1, the mode is at most N-1 or K, and log_p(N+1), log_p(K)
// and the tail's increment are closed form in L_N = log(serv_rate(N)).
struct LdsCompactTable {
  const double *cum;
  int N;
  double log_mu_n;  // L_N
  // the compare is on the double, so an N no int holds is rejected by
  // row_valid before any cast
  static __device__ bool fits(const double *pr, int max_n) {
    return trunc(pr[P_MAX_BATCH]) <= (double)max_n;
  }
  __device__ LdsCompactTable(const Parms &p, const double *table)
      : cum(table), N(p.max_batch), log_mu_n(log_mu(p, p.max_batch - 1)) {}
  __device__ int scan_length() const { return N; }
  __device__ int chain() const { return N * (1 + kMaxQueueToBatchRatio); }
  __device__ double log_p(double loglam, int n) const {
    return log_p_compact(cum, N, log_mu_n, loglam, n);
  }
  __device__ GeoTail tail(int, double loglam, double m, int *loop_hi) const {
    return geo_tail_compact(cum, N, log_mu_n, loglam, m, loop_hi);
  }
};

// One model evaluation by THREADS threads over a table in LDS.  With one
// wave (THREADS == 64) it is barrier-free and indexed by the LANE, so the
// waves of the dual and speculative kernels each run their own; with more
// it takes two workgroup barriers, which every thread must reach.
template <int THREADS, typename Table>
struct WgEval {
  static constexpr int WAVES = THREADS / 64;
  const Parms &p;
  Table table;
  double *red;  // LDS scratch, WAVES * 5 (unused with one wave)

  // Wave-parallel equivalent of log_mode_state (queue_core.h): same
  // boundary index, found with ballots instead of a per-lane serial
  // bisection.
  __device__ int mode_state_wave(int K, double lam, int lane) const {
    double tN = prefill_time(p, (double)p.max_batch) +
                p.num_decode * decode_time(p, (double)p.max_batch);
    if ((double)p.max_batch <= lam * tN) return K;
    double t1 = prefill_time(p, 1.0) + p.num_decode * decode_time(p, 1.0);
    if (lam * t1 <= 1.0) return 0;
    const int b = wave_lower_bound(
        1, p.max_batch, lane, [&](int i) { return !rate_below(p, i, lam); });
    return b - 1;
  }

  __device__ Stats eval(double lam) const {
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int K = table.chain();
    const double loglam = log(lam);

    // max of logp via the concavity closed form — wave-parallel
    // (ballot) in the single-wave geometry, scalar otherwise.  No
    // windowing: the pre-batch region is at most N+1 states (sub-
    // threshold terms just underflow toward 0 in the sweep, adding
    // accuracy, not cost) and the whole queue region [N+1, K] sums in
    // closed form below — so the two window boundary searches the
    // windowed design needed are gone entirely.
    int n_star;
    if constexpr (WAVES == 1) {
      n_star = mode_state_wave(K, lam, lane);
    } else {
      n_star = log_mode_state(p, K, lam);
    }
    double m = table.log_p(loglam, n_star);
    if (m < 0.0) m = 0.0;
    if constexpr (WAVES > 1) {
      __syncthreads();  // red may still be read from a previous eval
    }

    // single pass: normalization and moment sums (eK is the state-K
    // boundary term, reduced like the sums — only its owner thread
    // contributes a non-zero partial).  The geometric tail is uniform
    // across lanes and joins the reduced totals below.
    const int num = p.max_batch;
    const int idx = (WAVES == 1) ? lane : tid;
    int loop_hi;
    const GeoTail tail = table.tail(num, loglam, m, &loop_hi);
    double S = 0.0, Ni = 0.0, Snum = 0.0, Ninum = 0.0, eK = 0.0;
    // 2x-unrolled sweep: two independent exp chains in flight per lane
    // hide the fp64 transcendental latency the PMC profile flagged
    // (~34% issue-stall); accumulators are kept separate and combined
    // after the loop so the FLOATING-POINT SUM ORDER PER LANE CHANGES —
    // covered by the cross-geometry ulp-tolerance in the parity suite.
    {
      double S1 = 0.0, Ni1 = 0.0, Snum1 = 0.0, Ninum1 = 0.0, eK1 = 0.0;
      int n = idx;
      for (; n + THREADS <= loop_hi; n += 2 * THREADS) {
        const int n2 = n + THREADS;
        const double e = exp(table.log_p(loglam, n) - m);
        const double e2 = exp(table.log_p(loglam, n2) - m);
        S += e;
        Ni += (double)n * e;
        S1 += e2;
        Ni1 += (double)n2 * e2;
        if (n <= num) {
          Snum += e;
          Ninum += (double)n * e;
        }
        if (n2 <= num) {
          Snum1 += e2;
          Ninum1 += (double)n2 * e2;
        }
        if (n == K) eK = e;
        if (n2 == K) eK1 = e2;
      }
      if (n <= loop_hi) {
        const double e = exp(table.log_p(loglam, n) - m);
        S += e;
        Ni += (double)n * e;
        if (n <= num) {
          Snum += e;
          Ninum += (double)n * e;
        }
        if (n == K) eK = e;
      }
      S += S1;
      Ni += Ni1;
      Snum += Snum1;
      Ninum += Ninum1;
      eK += eK1;
    }
    for (int off = 32; off > 0; off >>= 1) {
      S += __shfl_down(S, off, 64);
      Ni += __shfl_down(Ni, off, 64);
      Snum += __shfl_down(Snum, off, 64);
      Ninum += __shfl_down(Ninum, off, 64);
      eK += __shfl_down(eK, off, 64);
    }
    if constexpr (WAVES == 1) {
      // single wave: broadcast lane 0's totals to every lane
      S = __shfl(S, 0, 64);
      Ni = __shfl(Ni, 0, 64);
      Snum = __shfl(Snum, 0, 64);
      Ninum = __shfl(Ninum, 0, 64);
      eK = __shfl(eK, 0, 64);
    } else {
      if (lane == 0) {
        red[wave * 5 + 0] = S;
        red[wave * 5 + 1] = Ni;
        red[wave * 5 + 2] = Snum;
        red[wave * 5 + 3] = Ninum;
        red[wave * 5 + 4] = eK;
      }
      __syncthreads();
      S = Ni = Snum = Ninum = eK = 0.0;
      for (int w = 0; w < WAVES; ++w) {
        S += red[w * 5 + 0];
        Ni += red[w * 5 + 1];
        Snum += red[w * 5 + 2];
        Ninum += red[w * 5 + 3];
        eK += red[w * 5 + 4];
      }
    }
    S += tail.S;
    Ni += tail.Ni;
    eK += tail.eK;
    return stats_of_sums(lam, num, S, Ni, Snum, Ninum, eK);
  }
};

// The row's cs^2: the launch's optional vector, indexed by the workgroup's
// row; a launch without one is Markovian (1.0), so stale bytes behind a
// reused buffer are never read.
__device__ inline double row_scv(const double *scv, int pid) {
  return scv != nullptr ? scv[pid] : 1.0;
}

// Row guard of every body, taken before anything touches LDS: true for a
// row that breaks the contract of queue_core.h (row_valid, which also wants
// the row's cs^2 finite and >= 0), or whose table does not fit the doubles
// this launch reserved for it.  Every thread of the workgroup reads the same
// row, so the early return it decides is uniform and precedes the first
// barrier.
template <typename Table>
__device__ inline bool row_rejected(const double *pr, double scv, int reserved) {
  return !(row_valid(pr, scv) & Table::fits(pr, reserved));
}

// Result stores.  Threads 0..RESULT_FIELDS-1 zero the row once, first thing
// in every body, and the same threads write a feasible row's values, one
// field each: both stores to a field come from one thread, in program
// order, and every exit in between leaves the all-zero row behind.
__device__ inline void zero_row(double *res) {
  if (threadIdx.x < RESULT_FIELDS) res[threadIdx.x] = 0.0;
}

__device__ inline void store_row(double *res, const RowValues vals) {
  const int tid = threadIdx.x;
  if (tid < RESULT_FIELDS) {
    double v = vals.feasible;
    v = (tid == R_REPLICAS) ? vals.replicas : v;
    v = (tid == R_RATE_STAR) ? vals.rate_star : v;
    v = (tid == R_ITL) ? vals.itl : v;
    v = (tid == R_TTFT) ? vals.ttft : v;
    v = (tid == R_RHO) ? vals.rho : v;
    res[tid] = v;
  }
}

// chunked parallel inclusive scan of log_mu over K states into LDS
template <int THREADS>
__device__ void build_cum(const Parms &p, int K, double *cum, double *totals) {
  const int tid = threadIdx.x;
  const int chunk = (K + THREADS - 1) / THREADS;
  const int lo = tid * chunk;
  const int hi = min(lo + chunk, K);
  double acc = 0.0;
  for (int n = lo; n < hi; ++n) {
    acc += log_mu(p, n);
    cum[n] = acc;
  }
  totals[tid] = (lo < K) ? acc : 0.0;
  __syncthreads();
  double offset = 0.0;
  for (int t = 0; t < tid; ++t) offset += totals[t];  // broadcast LDS reads
  for (int n = lo; n < hi; ++n) cum[n] += offset;
  __syncthreads();
}

// Sequential body: the whole workgroup evaluates one rate at a time and runs
// queue_core.h's solve_row in lockstep — every evaluation result is the same
// on all threads (broadcast reductions), so each search step, each
// infeasibility exit and the evaluator's barriers are reached uniformly.
// `reserved` is the table length the launch reserved LDS for (max_k for the
// full table, max_n for the compact one).
// LDS: cum[reserved], totals[THREADS], red[WAVES * 5] of the 64 slack doubles.
template <int THREADS, typename Table>
__device__ void solve_body(const double *__restrict__ prob,
                           const double *__restrict__ scv, double *__restrict__ out,
                           int n_problems, int reserved) {
  const int pid = blockIdx.x;
  if (pid >= n_problems) return;
  const double *pr = prob + (size_t)pid * PROBLEM_FIELDS;
  double *res = out + (size_t)pid * RESULT_FIELDS;

  const double cs2 = row_scv(scv, pid);
  zero_row(res);
  if (row_rejected<Table>(pr, cs2, reserved)) return;
  const Parms p = parms_from_problem(pr, cs2);

  extern __shared__ double smem[];
  double *cum = smem;                // this problem's table
  double *totals = smem + reserved;  // THREADS chunk totals
  double *red = totals + THREADS;

  const Table table(p, cum);
  build_cum<THREADS>(p, table.scan_length(), cum, totals);

  WgEval<THREADS, Table> ev{p, table, red};
  store_row(res, solve_row(pr, p, ev));
}

// The dual body's own bisection: queue_core.h's binary_search with the
// bracket classification written out and y(x_max) evaluated only after
// y(x_min) missed the target.  Same results, bit for bit; it is kept apart
// for speed alone.  Over the shared binary_search the dual kernel compiles
// to 127 registers instead of 133 and a different schedule, which measured
// 3-5 % slower at B = 4096, N = 256 (0.4556 against 0.4310 ms) — a shape it
// is the automatic pick for — though faster at N = 64 and 700.  With this
// text it matches the earlier kernel at all three (profiles/native_dedup.md).
// A change to the search has to be made in both.
template <typename F>
__device__ int wg_binary_search(double x_min, double x_max, double y_target, F eval,
                                double *x_star) {
  double y0 = eval(x_min);
  if (within_tolerance(y0, y_target, kTolerance)) {
    *x_star = x_min;
    return 0;
  }
  double y1 = eval(x_max);
  if (within_tolerance(y1, y_target, kTolerance)) {
    *x_star = x_max;
    return 0;
  }
  if (within_tolerance(y0, y1, kTolerance)) {
    // flat function: classify by value only (direction would be noise)
    if (y_target > fmax(y0, y1)) {
      *x_star = x_max;
      return +1;
    }
    *x_star = x_min;
    return -1;
  }
  bool increasing = y0 < y1;
  if ((increasing && y_target < y0) || (!increasing && y_target > y0)) {
    *x_star = x_min;
    return -1;
  }
  if ((increasing && y_target > y1) || (!increasing && y_target < y1)) {
    *x_star = x_max;
    return +1;
  }
  double xs = x_min;
  for (int i = 0; i < kMaxIterations; ++i) {
    xs = 0.5 * (x_min + x_max);
    double ys = eval(xs);
    if (within_tolerance(ys, y_target, kTolerance)) break;
    if ((increasing && y_target < ys) || (!increasing && y_target > ys)) {
      x_max = xs;
    } else {
      x_min = xs;
    }
  }
  *x_star = xs;
  return 0;
}

// 2-wave "dual" body: the TTFT and ITL bisections are independent, so
// wave 0 searches the TTFT target while wave 1 searches the ITL target
// concurrently.  Each wave's evaluations are the barrier-free one-wave
// WgEval (lane-indexed, __shfl-only), so the waves may diverge arbitrarily
// between the scan barrier and the exchange barrier.  Semantics are
// identical to the sequential body: the original runs TTFT first and
// returns infeasible without touching ITL — here both run, but the
// combined feasibility check and the zeroed result row give the same
// observable output.
__device__ void solve_body_dual(const double *__restrict__ prob,
                                const double *__restrict__ scv,
                                double *__restrict__ out, int n_problems, int max_k) {
  constexpr int THREADS = 128;
  const int pid = blockIdx.x;
  if (pid >= n_problems) return;
  const double *pr = prob + (size_t)pid * PROBLEM_FIELDS;
  double *res = out + (size_t)pid * RESULT_FIELDS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;

  const double cs2 = row_scv(scv, pid);
  zero_row(res);
  if (row_rejected<LdsFullTable>(pr, cs2, max_k)) return;
  const Parms p = parms_from_problem(pr, cs2);

  extern __shared__ double smem[];
  double *cum = smem;             // this problem's K entries
  double *totals = smem + max_k;  // THREADS chunk totals
  double *ex = totals + THREADS;  // exchange: lam_ttft, ind_ttft, lam_itl, ind_itl

  const LdsFullTable table(p, cum);
  build_cum<THREADS>(p, table.scan_length(), cum, totals);

  double lam_min, lam_max;
  rate_bracket(p, &lam_min, &lam_max);

  WgEval<64, LdsFullTable> ev{p, table, nullptr};

  double lam_t = lam_max;
  int ind = 0;
  if (wave == 0) {
    if (pr[P_TARGET_TTFT] > 0.0) {
      ind = wg_binary_search(
          lam_min, lam_max, pr[P_TARGET_TTFT],
          [&](double x) { return eval_ttft_of(p, ev.eval(x)); }, &lam_t);
    }
  } else {
    if (pr[P_TARGET_ITL] > 0.0) {
      ind = wg_binary_search(
          lam_min, lam_max, pr[P_TARGET_ITL],
          [&](double x) { return eval_itl_of(p, ev.eval(x)); }, &lam_t);
    }
  }
  if ((tid & 63) == 0) {
    ex[wave * 2 + 0] = lam_t;
    ex[wave * 2 + 1] = (double)ind;
  }
  __syncthreads();
  if (ex[1] < 0.0 || ex[3] < 0.0) return;  // a target below the reachable range
  if (wave == 1) return;                   // wave 0 finishes the tail alone

  store_row(res, row_tail(pr, p, ev, lam_max, ex[0], ex[2]));
}

// ---------------------------------------------------------------------------
// Speculative-tree multisection ("spec") kernel — round-2 lever
// (profiles/r01_rocprof_pmc.txt: ~32% of wave time parked at barriers and
// ~34% issue-stalled on the fp64 exp/log chain of the SEQUENTIAL model
// evaluations, up to 30 per target; the bisection itself is the critical
// path).
//
// Geometry: 2 search groups (TTFT, ITL) x SW waves, SW = 2^D - 1.  Each
// round every group evaluates the ENTIRE depth-D midpoint tree of its
// current bracket concurrently — candidate k (heap order) is the
// midpoint reached after the D halvings encoded by k's bits, computed by
// the same (lo+hi)/2 recurrence the sequential loop uses, so the
// iterates x are BITWISE identical to binary_search's and, over the
// same cum table, so is every y and the whole result.  Across geometries
// the table itself is not the same: build_cum's chunked scan adds log_mu
// in a THREADS-dependent order once K > 64, which moves y and the
// outputs by last-place bits (measured <= 2e-14 relative on MI355X; with
// fp contraction off as well, so that is not the cause) while the
// decision walk, feasibility and replica counts stay identical.  For
// K <= 64 every geometry scans one state per thread and the outputs of
// 64/128/384/896 are bit-identical (tests/test_ops_oracle.py pins both
// statements).  The group then replays the sequential
// decision walk on the cached y values, consuming D bisection levels per
// round: D=2 (SW=3, 384 threads) halves the serial rounds per target.
// kMaxIterations = 100 is only the cap: the 1e-6 stop ends a search after
// at most 30 evaluations (two of them the bracket ends; median 22) on the
// flagship benchmark's rows, counted with the Python analyzer on 1536 of
// them — so a target costs about one pre-phase round plus <= 14 tree
// rounds here.  6 resident waves per CU hide the exp chain latency the
// PMC profile flagged.
//
// Wave synchronization is group-local LDS mailboxes (publish y, fence,
// bump flag; consumers spin with s_sleep) — NO workgroup barriers after
// the scan, so the two searches never lock-step each other (the dual
// kernel's exchange barrier is gone too).
// ---------------------------------------------------------------------------

__device__ inline void mb_publish(volatile double *slot, double y,
                                  volatile double *flag, double round_id) {
  *slot = y;
  __threadfence_block();
  *flag = round_id;
}

// Watchdog: a legitimate wait is bounded by a sibling wave's evaluation
// (microseconds); ~16M sleep iterations is on the order of a second of
// GPU time.  If a (hypothetical) control-flow divergence bug ever broke
// the uniform-rounds invariant, the spin gives up instead of hanging
// the device — every wave of the group times out the same way, all
// fall through, and the problem's zeroed result row reads as
// infeasible: wrong-but-finite beats a dead GPU.
constexpr unsigned kMailboxSpinLimit = 1u << 24;

__device__ inline bool mb_wait(volatile double *flags, int n, double round_id) {
  for (int j = 0; j < n; ++j) {
    unsigned spins = 0;
    while (flags[j] < round_id) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > kMailboxSpinLimit) return false;
    }
  }
  __threadfence_block();
  return true;
}

// Midpoint at heap node k (1-based: 1 = root midpoint, 2/3 = children,
// 4..7 = grandchildren).  The bits of k below its leading 1 encode the
// left(0)/right(1) path; each step repeats the sequential loop's exact
// (lo+hi)/2 recurrence, so the value is BITWISE what the sequential
// bisection would compute on that path.
__device__ inline double heap_midpoint(double lo, double hi, int k) {
  double x = 0.5 * (lo + hi);
  const int depth_below = 31 - __clz(k);
  for (int level = depth_below - 1; level >= 0; --level) {
    if ((k >> level) & 1) {
      lo = x;
    } else {
      hi = x;
    }
    x = 0.5 * (lo + hi);
  }
  return x;
}

// Speculative bisection for one search group.  All SW waves of the group
// execute this with identical control flow; `sub` is the wave's index
// within the group, `yb`/`fl` its SW-slot mailbox.  Returns the boundary
// indicator (-1/0/+1) and writes lambda* like binary_search, whose bracket
// classification it shares (queue_core.h).
template <int D, typename F>
__device__ int spec_binary_search(double x_min, double x_max, double y_target,
                                  F eval, int sub, volatile double *yb,
                                  volatile double *fl, double *x_star) {
  constexpr int SW = (1 << D) - 1;
  const int lane = threadIdx.x & 63;

  // pre-phase: y(x_min) and y(x_max) evaluated concurrently (slots 0,1)
  double mine = 0.0;
  if (sub == 0) mine = eval(x_min);
  if (sub == 1) mine = eval(x_max);
  if (lane == 0 && sub < 2) mb_publish(&yb[sub], mine, &fl[sub], 1.0);
  if (!mb_wait(fl, 2, 1.0)) {  // watchdog: treat as unreachable target
    *x_star = x_min;
    return -1;
  }
  const double y0 = yb[0];
  const double y1 = yb[1];
  bool increasing = false;
  const int cls = classify_bracket(x_min, x_max, y0, y1, y_target, x_star, &increasing);
  if (cls != kBisect) return cls;

  double lo = x_min, hi = x_max, xs = x_min;
  double round_id = 2.0;
  int iters = 0;
  while (iters < kMaxIterations) {
    // evaluate the whole depth-D midpoint tree of [lo, hi]
    const double x_mine = heap_midpoint(lo, hi, sub + 1);
    const double y_mine = eval(x_mine);
    if (lane == 0) mb_publish(&yb[sub], y_mine, &fl[sub], round_id);
    if (!mb_wait(fl, SW, round_id)) {
      *x_star = x_min;
      return -1;
    }
    round_id += 1.0;

    // replay the sequential walk on the cached tree
    int k = 1;
    bool done = false;
    for (int level = 0; level < D && iters < kMaxIterations; ++level) {
      xs = 0.5 * (lo + hi);
      const double ys = yb[k - 1];
      ++iters;
      if (within_tolerance(ys, y_target, kTolerance)) {
        done = true;
        break;
      }
      if ((increasing && y_target < ys) || (!increasing && y_target > ys)) {
        hi = xs;
        k = 2 * k;
      } else {
        lo = xs;
        k = 2 * k + 1;
      }
    }
    if (done) break;
  }
  *x_star = xs;
  return 0;
}

// Mailbox LDS layout (doubles, after cum[max_k] + totals[THREADS]):
//   [0..6]   group-0 y slots      [7..13]  group-0 flags
//   [14..20] group-1 y slots      [21..27] group-1 flags
//   [28..31] results: lam0, ind0, lam1, ind1
//   [32..33] done flags per group
//   [40..47] depth 3 only: the row's Parms (see below)
template <int D>
__device__ void solve_body_spec(const double *__restrict__ prob,
                                const double *__restrict__ scv,
                                double *__restrict__ out, int n_problems,
                                int max_k) {
  constexpr int SW = (1 << D) - 1;
  constexpr int THREADS = 2 * SW * 64;
  const int pid = blockIdx.x;
  if (pid >= n_problems) return;
  const double *pr = prob + (size_t)pid * PROBLEM_FIELDS;
  double *res = out + (size_t)pid * RESULT_FIELDS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int group = wave / SW;   // 0 = TTFT, 1 = ITL
  const int sub = wave % SW;
  const int lane = tid & 63;

  const double cs2 = row_scv(scv, pid);
  zero_row(res);
  if (row_rejected<LdsFullTable>(pr, cs2, max_k)) return;
  const Parms p0 = parms_from_problem(pr, cs2);

  extern __shared__ double smem[];
  double *cum = smem;
  double *totals = smem + max_k;
  double *mail = totals + THREADS;
  if (tid < 34) mail[tid] = 0.0;
  // The 896-thread geometry has 128 vector registers per lane and spills:
  // there the searches read the row's constants from LDS (8 of the 64
  // slack doubles, published by the scan's closing barrier) instead of
  // holding all of them, wait_scale included, in registers.  Same values,
  // same arithmetic.
  static_assert(sizeof(Parms) <= 8 * sizeof(double), "Parms outgrew its LDS slot");
  const Parms *pp = &p0;
  if constexpr (D == 3) {
    Parms *shared_parms = reinterpret_cast<Parms *>(mail + 40);
    if (tid == 0) *shared_parms = p0;
    pp = shared_parms;
  }

  const LdsFullTable table(p0, cum);
  build_cum<THREADS>(p0, table.scan_length(), cum, totals);  // ends with __syncthreads()
  const Parms &p = *pp;

  double lam_min, lam_max;
  rate_bracket(p, &lam_min, &lam_max);

  WgEval<64, LdsFullTable> ev{p, table, nullptr};  // lane-indexed, barrier-free

  volatile double *yb = mail + group * 14;
  volatile double *fl = yb + 7;
  volatile double *ex = mail + 28;
  volatile double *done = mail + 32;

  double lam_t = lam_max;
  int ind = 0;
  const double target = (group == 0) ? pr[P_TARGET_TTFT] : pr[P_TARGET_ITL];
  if (target > 0.0) {
    if (group == 0) {
      ind = spec_binary_search<D>(
          lam_min, lam_max, target,
          [&](double x) { return eval_ttft_of(p, ev.eval(x)); }, sub, yb, fl, &lam_t);
    } else {
      ind = spec_binary_search<D>(
          lam_min, lam_max, target,
          [&](double x) { return eval_itl_of(p, ev.eval(x)); }, sub, yb, fl, &lam_t);
    }
  }
  if (sub == 0 && lane == 0) {
    ex[group * 2 + 0] = lam_t;
    ex[group * 2 + 1] = (double)ind;
    __threadfence_block();
    done[group] = 1.0;
  }
  if (wave != 0) return;  // group-0 wave 0 finishes the tail alone

  if (!mb_wait(done, 2, 1.0)) return;  // watchdog: leave result infeasible
  if (ex[1] < 0.0 || ex[3] < 0.0) return;  // a target below reachable range

  store_row(res, row_tail(pr, p, ev, lam_max, ex[0], ex[2]));
}

extern "C" __global__ void __launch_bounds__(384) wva_solve_kernel_384(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_k) {
  solve_body_spec<2>(prob, scv, out, n_problems, max_k);
}

extern "C" __global__ void __launch_bounds__(896) wva_solve_kernel_896(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_k) {
  solve_body_spec<3>(prob, scv, out, n_problems, max_k);
}

extern "C" __global__ void __launch_bounds__(256) wva_solve_kernel_256(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_k) {
  solve_body<256, LdsFullTable>(prob, scv, out, n_problems, max_k);
}

extern "C" __global__ void __launch_bounds__(64) wva_solve_kernel_64(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_k) {
  solve_body<64, LdsFullTable>(prob, scv, out, n_problems, max_k);
}

extern "C" __global__ void __launch_bounds__(128) wva_solve_kernel_128(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_k) {
  solve_body_dual(prob, scv, out, n_problems, max_k);
}

// Compact-table kernel: rows with max batch beyond the full table's LDS
// limit (N up to ~7800 instead of ~700).  One geometry: the sequential body
// at 256 threads over LdsCompactTable — build_cum over N states, scalar mode
// search, 4-wave strided sweeps with the LDS cross-wave combine, TTFT then
// ITL bisection.  LDS: (max_n + 256 + 64) doubles.
constexpr int kCompactThreads = 256;

extern "C" __global__ void __launch_bounds__(kCompactThreads) wva_solve_kernel_compact(
    const double *__restrict__ prob, const double *__restrict__ scv,
    double *__restrict__ out, int n_problems, int max_n) {
  solve_body<kCompactThreads, LdsCompactTable>(prob, scv, out, n_problems, max_n);
}

}  // namespace wva

#include <cstdlib>
#include <cstring>

namespace {

using SizingKernel = void (*)(const double *, const double *, double *, int, int);

struct Geometry {
  int threads;
  const char *name;  // the value of WVA_GPU_THREADS that forces it
  SizingKernel kernel;
};

enum { kSeq64, kDual128, kSeq256, kSpec384, kSpec896 };  // rows of kGeometries

const Geometry kGeometries[] = {
    {64, "64", wva::wva_solve_kernel_64},    {128, "128", wva::wva_solve_kernel_128},
    {256, "256", wva::wva_solve_kernel_256}, {384, "384", wva::wva_solve_kernel_384},
    {896, "896", wva::wva_solve_kernel_896},
};

// 64 KiB LDS per workgroup: the table, totals[threads] and 64 slack doubles
// (compared so that no table_len can overflow the sum)
bool fits_lds(int table_len, int threads) {
  return table_len <= 64 * 1024 / 8 - threads - 64;
}

// Returns 0 on success, -1 when the table is empty or the LDS footprint
// exceeds 64 KiB — decided BEFORE anything is launched, instead of issuing a
// launch that cannot start — or the hipError_t of a failed launch.
int launch(const Geometry &g, const double *prob, const double *scv, double *out,
           int n_problems, int table_len, void *stream) {
  if (table_len < 1 || !fits_lds(table_len, g.threads)) return -1;
  const size_t smem = (size_t)(table_len + g.threads + 64) * sizeof(double);
  hipLaunchKernelGGL(g.kernel, dim3(n_problems), dim3(g.threads), smem, (hipStream_t)stream,
                     prob, scv, out, n_problems, table_len);
  return (int)hipGetLastError();
}

}  // namespace

// Full-table launch; return values as launch() above (-1 for max_k beyond
// N ~ 715).  scv is the optional device vector of per-row service-time cs^2
// (n_problems doubles); nullptr launches the Markovian model.  It changes
// neither the geometry pick nor the LDS size.
extern "C" int wva_launch_solve_scv(const double *prob, const double *scv, double *out,
                                    int n_problems, int max_k, void *stream) {
  // WVA_GPU_THREADS=64|128|256|384|896 forces a geometry; anything else is
  // ignored.  A forced speculative geometry (384, 896) that does not fit
  // falls back to the automatic pick; a forced 64/128/256 that does not fit
  // is refused by launch().
  const Geometry *g = nullptr;
  if (const char *env = std::getenv("WVA_GPU_THREADS")) {
    for (const Geometry &listed : kGeometries) {
      if (std::strcmp(env, listed.name) == 0) g = &listed;
    }
  }
  if (g != nullptr && g->threads > 256 && !fits_lds(max_k, g->threads)) g = nullptr;
  if (g == nullptr) {
    // The automatic pick, on the launch size (measured:
    // profiles/r02_kernel_geo.json).
    //   - Chip-filling launches (B >= 512) are THROUGHPUT-bound: with the
    //     geometric queue-tail (queue_core.h geo_tail) collapsing the sweep
    //     cost, the dual kernel's 2 evaluations per round are the least
    //     redundant work at every measured chip-filling point — B=4096 rows:
    //     0.33/0.44/1.04 ms at K=704/2816/7700 vs spec-384's 0.75/1.01/1.21.
    //   - Underfilled launches can't occupy 256 CUs, so the serial bisection
    //     IS the runtime and the speculative-tree multisection kernel (depth
    //     2, 2 x 3 waves, 2 levels per round) wins every measured point:
    //     0.106/0.116/0.141 ms at B=192 K=704/2816/7700 (r01 best geometry:
    //     0.175/0.277/0.360).
    g = &kGeometries[n_problems >= 512 ? kDual128 : fits_lds(max_k, 384) ? kSpec384 : kSeq256];
  }
  return launch(*g, prob, scv, out, n_problems, max_k, stream);
}

// Compact-table launch: max_n is the largest trunc(N) the launch reserves
// LDS for (a row beyond it gets the all-zero row).  One geometry;
// WVA_GPU_THREADS does not apply.
extern "C" int wva_launch_solve_compact(const double *prob, const double *scv, double *out,
                                        int n_problems, int max_n, void *stream) {
  const Geometry compact{wva::kCompactThreads, "", wva::wva_solve_kernel_compact};
  return launch(compact, prob, scv, out, n_problems, max_n, stream);
}
