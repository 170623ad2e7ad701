// The one pybind11 wrapper of greedy_core.h, shared by the torch binding and
// the torch-free one (like scv_arg.h, they have no other header in common
// that may include pybind11).
//
// Inputs are one-dimensional contiguous buffers (array.array or numpy):
// int64 for capacity, priority, alloc_offset, num_replicas and
// units_per_replica, float64 for value, int32 for type_index.  Returns two
// lists with one int per server: the chosen allocation's index in the
// server's slice (-1: none) and the granted replicas.  The GIL stays held:
// the solve takes a few microseconds at fleet sizes, less than handing the
// interpreter over and back is worth.

#pragma once

#include <pybind11/pybind11.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "greedy_core.h"

namespace wva {
namespace greedy {

namespace py = pybind11;

template <typename T>
inline const T *flat(const py::buffer_info &info, const char *name, const char *formats,
                     int64_t length) {
  const bool format_ok =
      info.format.size() == 1 && std::string(formats).find(info.format[0]) != std::string::npos;
  if (!format_ok || info.itemsize != (py::ssize_t)sizeof(T))
    throw std::invalid_argument(std::string(name) + ": wrong element type");
  if (info.ndim != 1 || info.shape[0] != length ||
      (length > 1 && info.strides[0] != (py::ssize_t)sizeof(T)))
    throw std::invalid_argument(std::string(name) + ": must be contiguous, one-dimensional, of length " +
                                std::to_string(length));
  return static_cast<const T *>(info.ptr);
}

inline py::tuple greedy_solve(py::buffer capacity, py::buffer priority, py::buffer alloc_offset,
                              py::buffer value, py::buffer num_replicas, py::buffer type_index,
                              py::buffer units_per_replica, bool delayed_best_effort, int policy) {
  static const char *kInt64 = "qln", *kInt32 = "il", *kDouble = "d";
  const py::buffer_info cap = capacity.request(), pri = priority.request(),
                        off = alloc_offset.request(), val = value.request(),
                        rep = num_replicas.request(), typ = type_index.request(),
                        uni = units_per_replica.request();
  if (cap.ndim != 1 || pri.ndim != 1)
    throw std::invalid_argument("capacity and priority must be one-dimensional");
  const int64_t n_types = cap.shape[0], n_servers = pri.shape[0];
  if (n_types > INT32_MAX || n_servers > INT32_MAX) throw std::invalid_argument("too many rows");

  Problem p;
  p.n_types = (int)n_types;
  p.n_servers = (int)n_servers;
  p.capacity = flat<int64_t>(cap, "capacity", kInt64, n_types);
  p.priority = flat<int64_t>(pri, "priority", kInt64, n_servers);
  p.alloc_offset = flat<int64_t>(off, "alloc_offset", kInt64, n_servers + 1);
  if (p.alloc_offset[0] != 0 || p.alloc_offset[n_servers] < 0)
    throw std::invalid_argument("alloc_offset must run from 0 to the number of allocations");
  const int64_t n_allocs = p.alloc_offset[n_servers];
  p.value = flat<double>(val, "value", kDouble, n_allocs);
  p.num_replicas = flat<int64_t>(rep, "num_replicas", kInt64, n_allocs);
  p.type_index = flat<int32_t>(typ, "type_index", kInt32, n_allocs);
  p.units_per_replica = flat<int64_t>(uni, "units_per_replica", kInt64, n_allocs);
  p.delayed_best_effort = delayed_best_effort;
  p.policy = policy;
  if (const char *what = check(p)) throw std::invalid_argument(what);

  std::vector<int32_t> chosen((size_t)n_servers);
  std::vector<int64_t> granted((size_t)n_servers);
  solve(p, chosen.data(), granted.data());

  py::list chosen_out((size_t)n_servers), granted_out((size_t)n_servers);
  for (int64_t s = 0; s < n_servers; ++s) {
    chosen_out[(size_t)s] = py::int_((long long)chosen[(size_t)s]);
    granted_out[(size_t)s] = py::int_((long long)granted[(size_t)s]);
  }
  return py::make_tuple(chosen_out, granted_out);
}

inline void bind(py::module_ &m) {
  m.def("greedy_solve", &greedy_solve,
        "Limited-mode greedy solve over flat arrays (greedy_core.h); returns "
        "(chosen index per server or -1, granted replicas per server)",
        py::arg("capacity"), py::arg("priority"), py::arg("alloc_offset"), py::arg("value"),
        py::arg("num_replicas"), py::arg("type_index"), py::arg("units_per_replica"),
        py::arg("delayed_best_effort"), py::arg("policy"));
  m.attr("HAS_GREEDY") = true;
}

}  // namespace greedy
}  // namespace wva
