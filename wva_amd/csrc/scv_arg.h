// The optional per-row service-time cs^2 vector (queue_core.h, M/G/1
// correction) as every numpy entry point takes it: float64, C-contiguous,
// [B], never converted, or the call raises.  None is the Markovian model,
// bit-identical to all ones, and gives nullptr.  The pointer borrows from
// the caller's argument, which outlives the call.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <string>

namespace wva {

inline const double *scv_data(const pybind11::object &scv, int64_t B) {
  namespace py = pybind11;
  if (scv.is_none()) return nullptr;
  if (!py::isinstance<py::array_t<double>>(scv)) {
    throw py::type_error("scv must be a float64 array");
  }
  py::array v = py::reinterpret_borrow<py::array>(scv);
  if (v.ndim() != 1 || v.shape(0) != B) {
    throw py::value_error("scv must be [B] = [" + std::to_string(B) + "]");
  }
  if (!(v.flags() & py::array::c_style)) {
    throw py::value_error("scv must be C-contiguous");
  }
  return (const double *)v.data();
}

}  // namespace wva
