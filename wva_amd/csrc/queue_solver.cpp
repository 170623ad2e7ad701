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
static const double *scv_data(const c10::optional<torch::Tensor> &scv,
                              const torch::Tensor &problems) {
  if (!scv.has_value()) return nullptr;
  const torch::Tensor &v = *scv;
  const int64_t B = problems.size(0);
  TORCH_CHECK(v.scalar_type() == torch::kFloat64, "scv must be float64");
  TORCH_CHECK(v.dim() == 1 && v.size(0) == B, "scv must be [B] = [", B, "]");
  TORCH_CHECK(v.is_contiguous(), "scv must be contiguous");
  TORCH_CHECK(v.device() == problems.device(), "scv must be on the device of problems");
  return B > 0 ? v.data_ptr<double>() : nullptr;
}

// The host solve of a contiguous CPU batch over either table policy of
// queue_host.h; scratch is sized by the longest table in the batch.
template <typename Table>
static torch::Tensor solve_on_cpu(const torch::Tensor &problems, const double *scv_ptr) {
  const int64_t B = problems.size(0);
  auto out = torch::zeros({B, (int64_t)wva::RESULT_FIELDS}, problems.options());
  if (B == 0) return out;
  const double *pr = problems.data_ptr<double>();
  double *res = out.data_ptr<double>();
  const int table_len = wva::batch_table_length<Table>(pr, B);
  at::parallel_for(0, B, 1, [&](int64_t begin, int64_t end) {
    std::vector<double> cum((size_t)table_len);
    for (int64_t i = begin; i < end; ++i) {
      wva::solve_one<Table>(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                            cum.data(), scv_ptr ? scv_ptr[i] : 1.0);
    }
  });
  return out;
}

static torch::Tensor solve_allocations(torch::Tensor problems, int64_t max_k_hint = -1,
                                       c10::optional<torch::Tensor> scv = c10::nullopt) {
  check_problems(problems);
  problems = problems.contiguous();
  const double *scv_ptr = scv_data(scv, problems);
  if (!problems.is_cuda()) return solve_on_cpu<wva::HostFullTable>(problems, scv_ptr);

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
    torch::Tensor problems, c10::optional<torch::Tensor> scv = c10::nullopt) {
  check_problems(problems);
  TORCH_CHECK(!problems.is_cuda(), "solve_allocations_compact takes CPU tensors");
  problems = problems.contiguous();
  return solve_on_cpu<wva::HostCompactTable>(problems, scv_data(scv, problems));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "wva_amd native batched queue solver (CPU + gfx950 HIP)";
  m.def("solve_allocations", &solve_allocations,
        "Batched state-dependent M/M/1/K allocation sizing",
        pybind11::arg("problems"), pybind11::arg("max_k_hint") = -1,
        pybind11::arg("scv") = pybind11::none());
  m.def("solve_allocations_compact", &solve_allocations_compact,
        "The same sizing on the CPU over the compact table (N doubles per row)",
        pybind11::arg("problems"), pybind11::arg("scv") = pybind11::none());
  m.attr("PROBLEM_FIELDS") = (int)wva::PROBLEM_FIELDS;
  m.attr("RESULT_FIELDS") = (int)wva::RESULT_FIELDS;
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
  m.def("collect", &wva::dispatch::collect,
        "Wait (GIL released) for a ticket and return its float64 [B, 6] results",
        pybind11::arg("ticket"));
  m.def("dispatch_pool_stats", &wva::dispatch::pool_stats,
        "(slots, slots in flight) of the dispatch pool");
  m.attr("HAS_HIP") = true;
#else
  m.attr("HAS_HIP") = false;
#endif
}
