// The optional per-row service-time cs^2 vector (queue_core.h, M/G/1
// correction) as every numpy entry point takes it: float64, C-contiguous,
// [B], never converted, or the call raises.  None is the Markovian model,
// bit-identical to all ones, and gives nullptr.  The pointer borrows from
// the caller's argument, which outlives the call.  The optional per-row
// ttft_tail vector (queue_core.h, TTFT percentile) travels the same way;
// there None means 0 for every row.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <string>

namespace wva {

inline const double *row_vector_data(const pybind11::object &vec, int64_t B,
                                     const std::string &name) {
  namespace py = pybind11;
  if (vec.is_none()) return nullptr;
  if (!py::isinstance<py::array_t<double>>(vec)) {
    throw py::type_error(name + " must be a float64 array");
  }
  py::array v = py::reinterpret_borrow<py::array>(vec);
  if (v.ndim() != 1 || v.shape(0) != B) {
    throw py::value_error(name + " must be [B] = [" + std::to_string(B) + "]");
  }
  if (!(v.flags() & py::array::c_style)) {
    throw py::value_error(name + " must be C-contiguous");
  }
  return (const double *)v.data();
}

inline const double *scv_data(const pybind11::object &scv, int64_t B) {
  return row_vector_data(scv, B, "scv");
}

}  // namespace wva
