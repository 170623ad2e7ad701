// Torch-free batched allocation sizing: pybind11 + numpy + OpenMP.
//
// The controller container image is slim (no libtorch, no ROCm); this
// binding gives it the same native CPU sizing path as the full build by
// reusing queue_host.h verbatim.  Input/output are numpy float64 arrays
// with the layouts of queue_core.h ([B,12] problems -> [B,6] results).

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <vector>

#include "queue_host.h"
#include "scv_arg.h"

namespace py = pybind11;

// One body for both table policies of queue_host.h: the full table
// (solve_allocations) and the compact one, N doubles of scratch per row
// instead of 11 * N (solve_allocations_compact).  scv: scv_arg.h.
template <typename Table>
static py::array_t<double> solve_allocations(
    py::array_t<double, py::array::c_style | py::array::forcecast> problems,
    py::object scv) {
  auto buf = problems.request();
  if (buf.ndim != 2 || buf.shape[1] != (ssize_t)wva::PROBLEM_FIELDS)
    throw std::invalid_argument("problems must be [B, 12] float64");
  const ssize_t B = buf.shape[0];
  const double *scv_ptr = wva::scv_data(scv, B);
  auto out = py::array_t<double>({B, (ssize_t)wva::RESULT_FIELDS});
  auto out_buf = out.request();
  const double *pr = (const double *)buf.ptr;
  double *res = (double *)out_buf.ptr;
  for (ssize_t i = 0; i < B * (ssize_t)wva::RESULT_FIELDS; ++i) res[i] = 0.0;
  if (B == 0) return out;

  const int table_len = wva::batch_table_length<Table>(pr, B);
  {
    py::gil_scoped_release release;
#pragma omp parallel
    {
      std::vector<double> cum((size_t)table_len);
#pragma omp for schedule(dynamic, 8)
      for (ssize_t i = 0; i < B; ++i) {
        wva::solve_one<Table>(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                              cum.data(), scv_ptr ? scv_ptr[i] : 1.0);
      }
    }
  }
  return out;
}

PYBIND11_MODULE(_queue_native_cpu, m) {
  m.doc() = "wva_amd torch-free batched queue solver (CPU/OpenMP)";
  m.def("solve_allocations", &solve_allocations<wva::HostFullTable>,
        "Batched state-dependent M/M/1/K allocation sizing", py::arg("problems"),
        py::arg("scv") = py::none());
  m.def("solve_allocations_compact", &solve_allocations<wva::HostCompactTable>,
        "The same sizing over the compact table (N doubles per row)",
        py::arg("problems"), py::arg("scv") = py::none());
  m.attr("PROBLEM_FIELDS") = (int)wva::PROBLEM_FIELDS;
  m.attr("RESULT_FIELDS") = (int)wva::RESULT_FIELDS;
}
