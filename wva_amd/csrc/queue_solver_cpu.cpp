// Torch-free batched allocation sizing: pybind11 + numpy + OpenMP.
//
// The controller container image is slim (no libtorch, no ROCm); this
// binding gives it the same native CPU sizing path as the full build by
// reusing queue_host.h verbatim.  Input/output are numpy float64 arrays
// with the layouts of queue_core.h ([B,12] problems -> [B,6] results).

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "queue_host.h"

namespace py = pybind11;

// scv: optional per-row service-time cs^2 (queue_core.h, M/G/1 correction).
// Unlike problems it is never converted: float64, C-contiguous, [B], or the
// call raises.  None is the Markovian model, bit-identical to all ones.
static py::array_t<double> solve_allocations(
    py::array_t<double, py::array::c_style | py::array::forcecast> problems,
    py::object scv) {
  auto buf = problems.request();
  if (buf.ndim != 2 || buf.shape[1] != (ssize_t)wva::PROBLEM_FIELDS)
    throw std::invalid_argument("problems must be [B, 12] float64");
  const ssize_t B = buf.shape[0];
  const double *scv_ptr = nullptr;
  py::array scv_arr;  // keeps the vector alive while the GIL is released
  if (!scv.is_none()) {
    if (!py::isinstance<py::array_t<double>>(scv))
      throw py::type_error("scv must be a float64 array");
    scv_arr = py::reinterpret_borrow<py::array>(scv);
    if (scv_arr.ndim() != 1 || scv_arr.shape(0) != B)
      throw py::value_error("scv must be [B] = [" + std::to_string(B) + "]");
    if (!(scv_arr.flags() & py::array::c_style))
      throw py::value_error("scv must be C-contiguous");
    scv_ptr = (const double *)scv_arr.data();
  }
  auto out = py::array_t<double>({B, (ssize_t)wva::RESULT_FIELDS});
  auto out_buf = out.request();
  const double *pr = (const double *)buf.ptr;
  double *res = (double *)out_buf.ptr;
  for (ssize_t i = 0; i < B * (ssize_t)wva::RESULT_FIELDS; ++i) res[i] = 0.0;
  if (B == 0) return out;

  int max_k = 1;
  for (ssize_t i = 0; i < B; ++i) {
    int k = wva::row_chain_length(pr + i * wva::PROBLEM_FIELDS);  // 0 if invalid
    if (k > max_k) max_k = k;
  }

  {
    py::gil_scoped_release release;
#pragma omp parallel
    {
      std::vector<double> cum((size_t)max_k);
#pragma omp for schedule(dynamic, 8)
      for (ssize_t i = 0; i < B; ++i) {
        wva::solve_one(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                       cum.data(), scv_ptr ? scv_ptr[i] : 1.0);
      }
    }
  }
  return out;
}

// The same over the compact table (queue_host.h solve_one_compact): N doubles
// of scratch per row instead of 11 * N.  solve_allocations above is untouched.
static py::array_t<double> solve_allocations_compact(
    py::array_t<double, py::array::c_style | py::array::forcecast> problems,
    py::object scv) {
  auto buf = problems.request();
  if (buf.ndim != 2 || buf.shape[1] != (ssize_t)wva::PROBLEM_FIELDS)
    throw std::invalid_argument("problems must be [B, 12] float64");
  const ssize_t B = buf.shape[0];
  const double *scv_ptr = nullptr;
  py::array scv_arr;  // keeps the vector alive while the GIL is released
  if (!scv.is_none()) {
    if (!py::isinstance<py::array_t<double>>(scv))
      throw py::type_error("scv must be a float64 array");
    scv_arr = py::reinterpret_borrow<py::array>(scv);
    if (scv_arr.ndim() != 1 || scv_arr.shape(0) != B)
      throw py::value_error("scv must be [B] = [" + std::to_string(B) + "]");
    if (!(scv_arr.flags() & py::array::c_style))
      throw py::value_error("scv must be C-contiguous");
    scv_ptr = (const double *)scv_arr.data();
  }
  auto out = py::array_t<double>({B, (ssize_t)wva::RESULT_FIELDS});
  auto out_buf = out.request();
  const double *pr = (const double *)buf.ptr;
  double *res = (double *)out_buf.ptr;
  for (ssize_t i = 0; i < B * (ssize_t)wva::RESULT_FIELDS; ++i) res[i] = 0.0;
  if (B == 0) return out;

  int max_k = 1;  // here the table is N doubles per row
  for (ssize_t i = 0; i < B; ++i) {
    int k = wva::row_compact_length(pr + i * wva::PROBLEM_FIELDS);  // 0 if invalid
    if (k > max_k) max_k = k;
  }

  {
    py::gil_scoped_release release;
#pragma omp parallel
    {
      std::vector<double> cum((size_t)max_k);
#pragma omp for schedule(dynamic, 8)
      for (ssize_t i = 0; i < B; ++i) {
        wva::solve_one_compact(pr + i * wva::PROBLEM_FIELDS, res + i * wva::RESULT_FIELDS,
                       cum.data(), scv_ptr ? scv_ptr[i] : 1.0);
      }
    }
  }
  return out;
}

PYBIND11_MODULE(_queue_native_cpu, m) {
  m.doc() = "wva_amd torch-free batched queue solver (CPU/OpenMP)";
  m.def("solve_allocations", &solve_allocations,
        "Batched state-dependent M/M/1/K allocation sizing", py::arg("problems"),
        py::arg("scv") = py::none());
  m.def("solve_allocations_compact", &solve_allocations_compact,
        "The same sizing over the compact table (N doubles per row)",
        py::arg("problems"), py::arg("scv") = py::none());
  m.attr("PROBLEM_FIELDS") = (int)wva::PROBLEM_FIELDS;
  m.attr("RESULT_FIELDS") = (int)wva::RESULT_FIELDS;
}
