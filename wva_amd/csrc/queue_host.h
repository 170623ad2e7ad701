// Host-side scalar solve of one sizing problem, shared by the torch
// binding (queue_solver.cpp: CPU at::parallel_for + HIP dispatch glue)
// and the torch-free pybind11/numpy binding (queue_solver_cpu.cpp) used
// in the slim controller image.  Semantics mirror
// core.create_allocation's non-zero-load body (see queue_solver.cpp's
// header comment for the reference citation); the solve itself is
// queue_core.h's solve_row, here over a table in host memory.
#pragma once

#include <cmath>
#include <vector>

#include "queue_core.h"

namespace wva {

// Table length the compact policy needs for a row: trunc(N), 0 if invalid.
inline int row_compact_length(const double *pr) {
  return row_valid(pr) ? (int)pr[P_MAX_BATCH] : 0;
}

// inclusive sum cum[n] = sum_{i<=n} log_mu(i) over the first `len` states
inline void fill_cum(const Parms &p, int len, double *cum) {
  double acc = 0.0;
  for (int n = 0; n < len; ++n) {
    acc += log_mu(p, n);
    cum[n] = acc;
  }
}

// Table policies of solve_one: how long a row's table is, how it is filled,
// and which eval_model* reads it.  Each is an evaluator for solve_row.  The
// constructor WRITES the caller's scratch table (the log_mu scan) and the
// object then only reads it.

// K = 11 * N doubles, evaluated inside the significance window (state_window)
struct HostFullTable {
  static int length(const double *pr) { return row_chain_length(pr); }
  const Parms &p;
  const double *cum;
  int K;
  HostFullTable(const Parms &parms, double *table)
      : p(parms), cum(table), K(parms.max_batch * (1 + kMaxQueueToBatchRatio)) {
    fill_cum(p, K, table);
  }
  Stats eval(double lam) const { return eval_model(p, cum, K, lam); }
};

// N doubles (queue_core.h, "Compact table"); no window
struct HostCompactTable {
  static int length(const double *pr) { return row_compact_length(pr); }
  const Parms &p;
  const double *cum;
  double log_mu_n;
  HostCompactTable(const Parms &parms, double *table)
      : p(parms), cum(table), log_mu_n(log_mu(parms, parms.max_batch - 1)) {
    fill_cum(p, p.max_batch, table);
  }
  Stats eval(double lam) const { return eval_model_compact(p, cum, log_mu_n, lam); }
};

// Scalar solve of one problem (CPU path).  cum must hold Table::length(pr)
// doubles; a row that breaks the contract of queue_core.h yields the
// all-zero row and touches no table.  scv is the row's service-time cs^2
// (1.0: Markovian); it only enters through Parms::wait_scale in eval_ttft_of.
template <typename Table>
inline void solve_one(const double *pr, double *out, double *cum, double scv = 1.0) {
  for (int f = 0; f < RESULT_FIELDS; ++f) out[f] = 0.0;
  if (!row_valid(pr, scv)) return;
  const Parms p = parms_from_problem(pr, scv);
  const Table table(p, cum);  // fills cum: the O(table length) build happens here
  const RowValues vals = solve_row(pr, p, table);
  out[R_FEASIBLE] = vals.feasible;
  out[R_REPLICAS] = vals.replicas;
  out[R_RATE_STAR] = vals.rate_star;
  out[R_ITL] = vals.itl;
  out[R_TTFT] = vals.ttft;
  out[R_RHO] = vals.rho;
}

// Scratch one thread needs for any row of a batch: the longest table, >= 1.
template <typename Table>
inline int batch_table_length(const double *pr, long long rows) {
  int longest = 1;
  for (long long i = 0; i < rows; ++i) {
    const int len = Table::length(pr + i * PROBLEM_FIELDS);  // 0 if invalid
    if (len > longest) longest = len;
  }
  return longest;
}

}  // namespace wva
