// Batched allocation sizing: torch binding + CPU (at::parallel_for) path.
//
// One "problem" is the non-zero-load body of core.create_allocation
// (/root/reference/pkg/core/allocation.go:77-160 re-designed): given the
// linear perf parameters, request shape, batch limit and SLO targets,
// find the max per-replica rate meeting the targets, the replica count for
// the offered load, and the predicted ITL/TTFT/rho at the final rate.
//
// The GPU path (queue_solver_hip.hip) runs one workgroup per problem on
// gfx950, in a geometry of 64 to 896 threads that its launcher picks; this
// file provides the same math on CPU and the dispatch glue.

#include <torch/extension.h>

#ifdef WVA_WITH_HIP
#include <c10/hip/HIPStream.h>
#endif

#include <climits>
#include <cmath>
#include <vector>


// Host scalar solve + bisection shared with the torch-free binding.
#include "queue_host.h"

// Limited-mode greedy solve, the same wrapper as in the torch-free binding.
#include "greedy_py.h"

#ifdef WVA_WITH_HIP
// 0 = launched; -1 = no kernel geometry fits max_k in LDS (nothing was
// launched); otherwise the hipError_t of the failed launch.  scv: one
// service-time cs^2 per row (device pointer), nullptr for the Markovian model
extern "C" int wva_launch_solve_scv(const double *prob, const double *scv, double *out,
                                    int n_problems, int max_k, void *stream);

// submit/collect on numpy arrays: the asynchronous, copy-light way into
// the same launcher (what wva_amd/ops/batched.py uses on the GPU)
#include "sizing_dispatch.h"
#endif

static void check_problems(const torch::Tensor &problems) {
  TORCH_CHECK(problems.dim() == 2 && problems.size(1) == wva::PROBLEM_FIELDS,
              "problems must be [B, ", (int)wva::PROBLEM_FIELDS, "]");
  TORCH_CHECK(problems.scalar_type() == torch::kFloat64, "problems must be float64");
}

// scv: optional per-row service-time cs^2 (queue_core.h, M/G/1 correction):
// float64, contiguous, [B], on the device of problems.  Absent is the
// Markovian model, bit-identical to a vector of ones, and gives nullptr.
// ttft_tail (queue_core.h, TTFT percentile) travels the same way; absent is
// 0 for every row, the mean TTFT.
static const double *scv_data(const c10::optional<torch::Tensor> &scv,
                              const torch::Tensor &problems, const char *name = "scv") {
  if (!scv.has_value()) return nullptr;
  const torch::Tensor &v = *scv;
  const int64_t B = problems.size(0);
  TORCH_CHECK(v.scalar_type() == torch::kFloat64, name, " must be float64");
  TORCH_CHECK(v.dim() == 1 && v.size(0) == B, name, " must be [B] = [", B, "]");
  TORCH_CHECK(v.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(v.device() == problems.device(), name, " must be on the device of problems");
  return B > 0 ? v.data_ptr<double>() : nullptr;
}

// The host solve of a contiguous CPU batch over either table policy of
// queue_host.h; scratch is sized by the longest table in the batch.
template <typename Table>
static torch::Tensor solve_on_cpu(const torch::Tensor &problems, const double *scv_ptr,
                                  const double *tail_ptr) {
  const int64_t B = problems.size(0);
  auto out = torch::zeros({B, (int64_t)wva::RESULT_FIELDS}, problems.options());
  if (B == 0) return out;
  const double *pr = problems.data_ptr<double>();
  double *res = out.data_ptr<double>();
  const int table_len = wva::batch_table_length<Table>(pr, B);
  const std::vector<double> lf = wva::log_factorials(wva::batch_tail_length<Table>(pr, tail_ptr, B));
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<double> cum((size_t)table_len);
    for (int64_t i = begin; i < end; ++i) {
      wva::solve_one<Table>(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                            cum.data(), scv_ptr ? scv_ptr[i] : 1.0,
                            tail_ptr ? tail_ptr[i] : 0.0, lf.data());
    }
  });
  return out;
}

static torch::Tensor solve_allocations(torch::Tensor problems, int64_t max_k_hint = -1,
                                       c10::optional<torch::Tensor> scv = c10::nullopt,
                                       c10::optional<torch::Tensor> ttft_tail = c10::nullopt) {
  check_problems(problems);
  problems = problems.contiguous();
  const double *scv_ptr = scv_data(scv, problems);
  const double *tail_ptr = scv_data(ttft_tail, problems, "ttft_tail");
  if (!problems.is_cuda()) {
    return solve_on_cpu<wva::HostFullTable>(problems, scv_ptr, tail_ptr);
  }
  // the full-table kernels size to the mean TTFT alone
  TORCH_CHECK(!ttft_tail.has_value(),
              "ttft_tail on the GPU goes through submit_tail, not solve_allocations");

  // the GPU kernels write all six fields of every row (rejected rows
  // included), so the output needs no zeroing
  const int64_t B = problems.size(0);
  auto out = torch::empty({B, (int64_t)wva::RESULT_FIELDS}, problems.options());
  if (B == 0) return out;
#ifdef WVA_WITH_HIP
  int max_k;
  if (max_k_hint > 0) {
    // caller-supplied chain length (hipGraph capture cannot tolerate
    // the .item() device sync below; wva_amd/ops/batched.py computes
    // it host-side from the numpy batch before upload).  The hint is
    // the LDS the launch reserves for the cumulative table; the kernels
    // check every row against it, so a hint that is too small for a row
    // yields the all-zero infeasible row for it, not corruption.
    max_k = max_k_hint > INT_MAX ? INT_MAX : (int)max_k_hint;
  } else {
    // largest N among the rows whose N is in the valid range: a NaN,
    // infinite or out-of-range N is an invalid row (queue_core.h) and
    // must not size the launch
    auto n = problems.select(1, wva::P_MAX_BATCH);
    auto in_range = n.ge(1.0).logical_and(n.lt((double)wva::kMaxBatchLimit + 1.0));
    const double max_batch =
        torch::where(in_range, n, torch::ones_like(n)).max().item<double>();
    max_k = (int)max_batch * (1 + wva::kMaxQueueToBatchRatio);
  }
  auto stream = c10::hip::getCurrentHIPStream();
  // the launcher picks the geometry and sizes its LDS before launching
  const int status = wva_launch_solve_scv(problems.data_ptr<double>(), scv_ptr,
                                          out.data_ptr<double>(), (int)B, max_k,
                                          (void *)stream.stream());
  TORCH_CHECK(status != -1,
              "max_batch too large for the LDS-resident GPU path (limit ~700, "
              "chain length ", max_k, "); use the CPU path for these problems");
  TORCH_CHECK(status == 0, "wva sizing kernel launch failed: ",
              hipGetErrorString((hipError_t)status));
  return out;
#else
  TORCH_CHECK(false, "wva native extension built without HIP support");
  return out;
#endif
}

// The host solve over the compact table: N doubles of scratch per row
// instead of 11 * N.  CPU tensors only; on the GPU the compact kernel is
// reached through submit_compact.
static torch::Tensor solve_allocations_compact(
    torch::Tensor problems, c10::optional<torch::Tensor> scv = c10::nullopt,
    c10::optional<torch::Tensor> ttft_tail = c10::nullopt) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "solve_allocations_compact takes CPU tensors");
  problems = problems.contiguous();
  return solve_on_cpu<wva::HostCompactTable>(problems, scv_data(scv, problems),
                                             scv_data(ttft_tail, problems, "ttft_tail"));
}

// The compact-table host solve with the waiting-time tail by the Poisson
// recurrence (queue_core.h, tail_sum_chunk), no log-factorial table: the host
// reference of the compact tail kernel, which is reached through
// submit_tail_compact.  CPU tensors only.
static torch::Tensor solve_allocations_tail_compact(
    torch::Tensor problems, c10::optional<torch::Tensor> scv = c10::nullopt,
    c10::optional<torch::Tensor> ttft_tail = c10::nullopt) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "solve_allocations_tail_compact takes CPU tensors");
  problems = problems.contiguous();
  return solve_on_cpu<wva::HostTailCompactTable>(problems, scv_data(scv, problems),
                                                 scv_data(ttft_tail, problems, "ttft_tail"));
}

// solve_allocations_tail_compact with one more optional vector, the rows'
// itl_tail (queue_core.h, "ITL percentile"): the host reference of the
// percentile kernel, which is reached through submit_ptile, and the CPU route
// of the rows that carry one.  CPU tensors only.
static torch::Tensor solve_allocations_ptile(
    torch::Tensor problems, c10::optional<torch::Tensor> scv = c10::nullopt,
    c10::optional<torch::Tensor> ttft_tail = c10::nullopt,
    c10::optional<torch::Tensor> itl_tail = c10::nullopt) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "solve_allocations_ptile takes CPU tensors");
  problems = problems.contiguous();
  const double *scv_ptr = scv_data(scv, problems);
  const double *tail_ptr = scv_data(ttft_tail, problems, "ttft_tail");
  const double *itl_ptr = scv_data(itl_tail, problems, "itl_tail");
  const int64_t B = problems.size(0);
  auto out = torch::zeros({B, (int64_t)wva::RESULT_FIELDS}, problems.options());
  if (B == 0) return out;
  const double *pr = problems.data_ptr<double>();
  double *res = out.data_ptr<double>();
  const int table_len = wva::batch_table_length<wva::HostCompactTable>(pr, B);
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<double> cum((size_t)table_len);
    for (int64_t i = begin; i < end; ++i) {
      wva::solve_one_ptile(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                           cum.data(), scv_ptr ? scv_ptr[i] : 1.0,
                           tail_ptr ? tail_ptr[i] : 0.0, itl_ptr ? itl_ptr[i] : 0.0);
    }
  });
  return out;
}

// The TTFT quantile of every row at its own rate and eps (queue_core.h, "TTFT
// quantile"), on the host: [B, 12] problems, float64 [B] rates (req/s per
// replica) and eps, optional scv -> [B, 2] (valid, q).  CPU tensors only; on
// the GPU the quantile kernels are reached through submit_quantile and
// submit_quantile_compact.  kCompact: quantile_one_compact, the table-free
// host reference of the compact quantile kernel, instead of quantile_one.
template <bool kCompact>
static torch::Tensor ttft_quantiles(torch::Tensor problems, torch::Tensor rates,
                                    torch::Tensor eps,
                                    c10::optional<torch::Tensor> scv = c10::nullopt) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "ttft_quantiles takes CPU tensors");
  problems = problems.contiguous();
  const int64_t B = problems.size(0);
  auto out = torch::zeros({B, (int64_t)wva::QUANTILE_FIELDS}, problems.options());
  const double *rate_ptr = scv_data(rates, problems, "rates");
  const double *eps_ptr = scv_data(eps, problems, "eps");
  const double *scv_ptr = scv_data(scv, problems);
  if (B == 0) return out;
  const double *pr = problems.data_ptr<double>();
  double *res = out.data_ptr<double>();
  const int table_len = wva::batch_table_length<wva::HostCompactTable>(pr, B);
  const std::vector<double> lf =
      wva::log_factorials(kCompact ? 0 : wva::quantile_tail_length(pr, B));
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<double> cum((size_t)table_len);
    for (int64_t i = begin; i < end; ++i) {
      const double *row = pr + i * wva::PROBLEM_FIELDS;
      double *q = res + i * wva::QUANTILE_FIELDS;
      const double cs2 = scv_ptr ? scv_ptr[i] : 1.0;
      if constexpr (kCompact) {
        wva::quantile_one_compact(row, rate_ptr[i], eps_ptr[i], q, cum.data(), cs2);
      } else {
        wva::quantile_one(row, rate_ptr[i], eps_ptr[i], q, cum.data(), lf.data(), cs2);
      }
    }
  });
  return out;
}

// The ITL quantile of every row at its own rate and eps (queue_core.h, "ITL
// quantile"), on the host: [B, 12] problems, float64 [B] rates (req/s per
// replica) and eps -> [B, 2] (valid, q).  CPU tensors only; on the GPU the ITL
// quantile kernel is reached through submit_itl_quantile.
static torch::Tensor itl_quantiles(torch::Tensor problems, torch::Tensor rates,
                                   torch::Tensor eps) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "itl_quantiles takes CPU tensors");
  problems = problems.contiguous();
  const int64_t B = problems.size(0);
  auto out = torch::zeros({B, (int64_t)wva::QUANTILE_FIELDS}, problems.options());
  const double *rate_ptr = scv_data(rates, problems, "rates");
  const double *eps_ptr = scv_data(eps, problems, "eps");
  if (B == 0) return out;
  const double *pr = problems.data_ptr<double>();
  double *res = out.data_ptr<double>();
  const int table_len = wva::batch_table_length<wva::HostCompactTable>(pr, B);
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<double> cum((size_t)table_len), suffix((size_t)table_len);
    for (int64_t i = begin; i < end; ++i) {
      wva::itl_quantile_one(pr + i * wva::PROBLEM_FIELDS, rate_ptr[i], eps_ptr[i],
                            res + i * wva::QUANTILE_FIELDS, cum.data(), suffix.data());
    }
  });
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "wva_amd native batched queue solver (CPU + gfx950 HIP)";
  m.def("solve_allocations", &solve_allocations,
        "Batched state-dependent M/M/1/K allocation sizing",
        pybind11::arg("problems"), pybind11::arg("max_k_hint") = -1,
        pybind11::arg("scv") = pybind11::none(), pybind11::arg("ttft_tail") = pybind11::none());
  m.def("solve_allocations_compact", &solve_allocations_compact,
        "The same sizing on the CPU over the compact table (N doubles per row)",
        pybind11::arg("problems"), pybind11::arg("scv") = pybind11::none(),
        pybind11::arg("ttft_tail") = pybind11::none());
  m.def("solve_allocations_tail_compact", &solve_allocations_tail_compact,
        "The compact-table sizing on the CPU with the waiting-time tail by the "
        "Poisson recurrence, no log-factorial table",
        pybind11::arg("problems"), pybind11::arg("scv") = pybind11::none(),
        pybind11::arg("ttft_tail") = pybind11::none());
  m.def("solve_allocations_ptile", &solve_allocations_ptile,
        "solve_allocations_tail_compact with the rows' itl_tail: the ITL search on "
        "the occupancy tail, the host reference of the percentile kernel",
        pybind11::arg("problems"), pybind11::arg("scv") = pybind11::none(),
        pybind11::arg("ttft_tail") = pybind11::none(),
        pybind11::arg("itl_tail") = pybind11::none());
  m.def("ttft_quantiles", &ttft_quantiles<false>,
        "The TTFT each row exceeds with probability eps at its per-replica rate "
        "(req/s), on the CPU: float64 [B, 2] of (valid, q in ms)",
        pybind11::arg("problems"), pybind11::arg("rates"), pybind11::arg("eps"),
        pybind11::arg("scv") = pybind11::none());
  m.def("ttft_quantiles_compact", &ttft_quantiles<true>,
        "ttft_quantiles without a log-factorial table: the host reference of the "
        "compact quantile kernel",
        pybind11::arg("problems"), pybind11::arg("rates"), pybind11::arg("eps"),
        pybind11::arg("scv") = pybind11::none());
  m.def("itl_quantiles", &itl_quantiles,
        "The ITL a share eps of each row's tokens exceeds at its per-replica rate "
        "(req/s), on the CPU: float64 [B, 2] of (valid, q in ms)",
        pybind11::arg("problems"), pybind11::arg("rates"), pybind11::arg("eps"));
  m.attr("PROBLEM_FIELDS") = (int)wva::PROBLEM_FIELDS;
  m.attr("RESULT_FIELDS") = (int)wva::RESULT_FIELDS;
  // greedy_solve, HAS_GREEDY
  wva::greedy::bind(m);
#ifdef WVA_WITH_HIP
  m.def("submit", &wva::dispatch::submit,
        "Enqueue upload, sizing kernel and download for a float64 [B, 12] "
        "numpy array (and an optional float64 [B] vector of per-row "
        "service-time cs^2) on the private dispatch stream; returns a ticket "
        "without waiting",
        pybind11::arg("problems"), pybind11::arg("max_k"),
        pybind11::arg("scv") = pybind11::none());
  m.def("submit_compact", &wva::dispatch::submit_compact,
        "submit through the compact-table kernel: max_n is the largest max "
        "batch N the launch reserves LDS for (N doubles, up to ~7800); same "
        "slot pool, stream, checks and collect as submit",
        pybind11::arg("problems"), pybind11::arg("max_n"),
        pybind11::arg("scv") = pybind11::none());
  m.def("submit_tail", &wva::dispatch::submit_tail,
        "submit through the waiting-time tail kernel: rows sized to a TTFT "
        "percentile, tail the float64 [B] vector of their ttft_tail; max_n is "
        "the largest max batch N the launch reserves LDS for (11 * N doubles, "
        "up to 700); same slot pool, stream, checks and collect as submit",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("tail"),
        pybind11::arg("scv") = pybind11::none());
  m.def("submit_tail_compact", &wva::dispatch::submit_tail_compact,
        "submit through the compact waiting-time tail kernel: rows sized to a "
        "TTFT percentile without a log-factorial table, tail the float64 [B] "
        "vector of their ttft_tail; max_n is the largest max batch N the launch "
        "reserves LDS for (N doubles, up to ~7800); same slot pool, stream, "
        "checks and collect as submit",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("tail"),
        pybind11::arg("scv") = pybind11::none());
  m.def("submit_quantile", &wva::dispatch::submit_quantile,
        "submit through the TTFT quantile kernel: rates (req/s per replica) and "
        "eps are float64 [B] vectors; max_n is the largest max batch N the "
        "launch reserves LDS for (10 * N doubles, up to 700); collect returns "
        "[B, 2] of (valid, q in ms) for such a ticket",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("rates"),
        pybind11::arg("eps"), pybind11::arg("scv") = pybind11::none());
  m.def("submit_quantile_compact", &wva::dispatch::submit_quantile_compact,
        "submit_quantile through the compact TTFT quantile kernel, which keeps no "
        "table of the tail sum: max_n is the largest max batch N the launch "
        "reserves LDS for (N doubles, up to ~7800)",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("rates"),
        pybind11::arg("eps"), pybind11::arg("scv") = pybind11::none());
  m.def("submit_itl_quantile", &wva::dispatch::submit_itl_quantile,
        "submit through the ITL quantile kernel: rates (req/s per replica) and eps "
        "are float64 [B] vectors; max_n is the largest max batch N the launch "
        "reserves LDS for (N doubles, up to 7872); collect returns [B, 2] of "
        "(valid, q in ms) for such a ticket",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("rates"),
        pybind11::arg("eps"));
  m.def("submit_ptile", &wva::dispatch::submit_ptile,
        "submit through the percentile kernel: rows whose ITL target is sized on "
        "the occupancy tail, itl_tail the float64 [B] vector of their allowed "
        "token share (required), ttft_tail the optional vector of the TTFT side; "
        "max_n is the largest max batch N the launch reserves LDS for (N doubles, "
        "up to 7872); split=True runs the measured alternative, both searches side "
        "by side on one wave each; same slot pool, stream, checks and collect as submit",
        pybind11::arg("problems"), pybind11::arg("max_n"), pybind11::arg("itl_tail"),
        pybind11::arg("ttft_tail") = pybind11::none(), pybind11::arg("scv") = pybind11::none(),
        pybind11::arg("split") = false);
  m.def("collect", &wva::dispatch::collect,
        "Wait (GIL released) for a ticket and return its float64 results: [B, 6], "
        "or [B, 2] for a submit_quantile, submit_quantile_compact or "
        "submit_itl_quantile ticket",
        pybind11::arg("ticket"));
  m.def("dispatch_pool_stats", &wva::dispatch::pool_stats,
        "(slots, slots in flight) of the dispatch pool");
  m.attr("HAS_HIP") = true;
#else
  m.attr("HAS_HIP") = false;
#endif
}
