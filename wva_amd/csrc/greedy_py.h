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
//
// greedy_solve_objects, further down, is the same solve with the per-
// allocation arrays read from the servers' Allocation objects instead
// (greedy_objects.h keeps the layout and the bounds, free of pybind11).

#pragma once

#include <pybind11/pybind11.h>
#include <structmember.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "greedy_core.h"
#include "greedy_objects.h"

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

// ---------------------------------------------------------------------------
// The same solve with the inputs read from the servers' Allocation objects
// (greedy.py: _solve_objects).  Everything here that touches a Python object
// is a C API call on an object whose exact type was checked first: an exact
// dict with exact str keys, values whose type is exactly `allocation_type`
// (a __slots__ class: its fields are loaded from their slots), exact float or
// int fields.  None of this runs Python code or allocates a tracked object,
// so no dict can change while it is walked.  Anything else, and
// anything outside the Builder's bounds, returns None: the caller then takes
// the array route, whose _marshal decides between greedy_solve and the
// Python body as it always did.  No error leaves this function for a reason
// that lies in the servers' data.

namespace detail {

struct Names {
  PyObject *all_allocations, *model_name, *value, *num_replicas, *accelerator;
};

inline const Names &names() {
  static const Names n = {
      PyUnicode_InternFromString("all_allocations"), PyUnicode_InternFromString("model_name"),
      PyUnicode_InternFromString("value"), PyUnicode_InternFromString("num_replicas"),
      PyUnicode_InternFromString("accelerator")};
  return n;
}

// an exact int that fits int64; false otherwise, with no error left set
inline bool exact_int64(PyObject *o, int64_t *out) {
  if (!PyLong_CheckExact(o)) return false;
  int overflow = 0;
  const long long v = PyLong_AsLongLongAndOverflow(o, &overflow);
  if (overflow != 0) return false;
  if (v == -1 && PyErr_Occurred()) {
    PyErr_Clear();
    return false;
  }
  *out = (int64_t)v;
  return true;
}

// an exact float, or an exact int as array('d') converts it
inline bool exact_double(PyObject *o, double *out) {
  if (PyFloat_CheckExact(o)) {
    *out = PyFloat_AS_DOUBLE(o);
    return true;
  }
  if (!PyLong_CheckExact(o)) return false;
  const double v = PyLong_AsDouble(o);
  if (v == -1.0 && PyErr_Occurred()) {
    PyErr_Clear();
    return false;
  }
  *out = v;
  return true;
}

// an attribute of a server: a new reference, or null with no error left set
inline py::object field(PyObject *o, PyObject *name) {
  PyObject *v = PyObject_GetAttr(o, name);
  if (v == nullptr) PyErr_Clear();
  return py::reinterpret_steal<py::object>(v);
}

// dict[key] for an exact dict and an exact str key: borrowed, or null
inline PyObject *lookup(PyObject *dict, PyObject *key) {
  PyObject *v = PyDict_GetItemWithError(dict, key);
  if (v == nullptr && PyErr_Occurred()) PyErr_Clear();
  return v;
}

// Where the instances of a __slots__ class keep the field `name`: the offset
// of the class's own member descriptor, or -1 when the class has none of
// that kind.  Reading the slot of an object of exactly that class is then a
// load: no descriptor call, no new reference, a null for an unset slot.
inline py::ssize_t slot_offset(PyTypeObject *type, PyObject *name) {
#if PY_VERSION_HEX >= 0x030C0000
  const py::object dict = py::reinterpret_steal<py::object>(PyType_GetDict(type));
  PyObject *d = dict ? lookup(dict.ptr(), name) : nullptr;
#else
  PyObject *d = type->tp_dict ? lookup(type->tp_dict, name) : nullptr;
#endif
  if (d == nullptr || Py_TYPE(d) != &PyMemberDescr_Type) return -1;
  const PyMemberDescrObject *descr = reinterpret_cast<PyMemberDescrObject *>(d);
  if (descr->d_common.d_type != type || descr->d_member->type != T_OBJECT_EX) return -1;
  return descr->d_member->offset;
}

inline PyObject *slot(PyObject *o, py::ssize_t offset) {
  return *reinterpret_cast<PyObject **>(reinterpret_cast<char *>(o) + offset);
}

}  // namespace detail

inline py::object greedy_solve_objects(py::list servers, py::list priority, py::buffer capacity,
                                       py::dict types, py::dict units, py::object allocation_type,
                                       bool delayed_best_effort, int policy) {
  static const char *kInt64 = "qln";
  const detail::Names &names = detail::names();
  const py::buffer_info cap = capacity.request();
  if (cap.ndim != 1) throw std::invalid_argument("capacity must be one-dimensional");
  const int64_t n_types = cap.shape[0];
  const py::ssize_t n_servers = PyList_GET_SIZE(servers.ptr());
  if (n_types > INT32_MAX || n_servers > INT32_MAX) throw std::invalid_argument("too many rows");
  if (PyList_GET_SIZE(priority.ptr()) != n_servers)
    throw std::invalid_argument("priority must have one entry per server");
  if (!PyType_Check(allocation_type.ptr()))
    throw std::invalid_argument("allocation_type must be a class");
  const int64_t *capacity_data = flat<int64_t>(cap, "capacity", kInt64, n_types);
  if (!PyDict_CheckExact(types.ptr()) || !PyDict_CheckExact(units.ptr())) return py::none();
  PyTypeObject *exact = reinterpret_cast<PyTypeObject *>(allocation_type.ptr());
  const py::ssize_t at_value = detail::slot_offset(exact, names.value),
                    at_replicas = detail::slot_offset(exact, names.num_replicas),
                    at_accelerator = detail::slot_offset(exact, names.accelerator);
  if (at_value < 0 || at_replicas < 0 || at_accelerator < 0) return py::none();

  Builder b;
  b.reserve((size_t)n_servers, (size_t)n_servers * 4);
  py::list candidates;  // every server's allocations, in order
  for (py::ssize_t s = 0; s < n_servers; ++s) {
    PyObject *server = PyList_GET_ITEM(servers.ptr(), s);
    int64_t prio = 0;
    if (!detail::exact_int64(PyList_GET_ITEM(priority.ptr(), s), &prio)) return py::none();
    // attribute reads on the server may run its class's code: they come
    // before its dict is walked, never during
    const py::object allocs = detail::field(server, names.all_allocations);
    if (!allocs || !PyDict_CheckExact(allocs.ptr())) return py::none();
    if (PyDict_GET_SIZE(allocs.ptr()) == 0) {
      b.end_server(prio);
      continue;
    }
    const py::object model_name = detail::field(server, names.model_name);
    if (!model_name || !PyUnicode_CheckExact(model_name.ptr())) return py::none();
    PyObject *model_units = detail::lookup(units.ptr(), model_name.ptr());
    if (model_units == nullptr || !PyDict_CheckExact(model_units)) return py::none();

    PyObject *key = nullptr, *alloc = nullptr;
    py::ssize_t pos = 0;
    while (PyDict_Next(allocs.ptr(), &pos, &key, &alloc)) {
      if (Py_TYPE(alloc) != exact) return py::none();
      PyObject *value = detail::slot(alloc, at_value), *replicas = detail::slot(alloc, at_replicas),
               *accelerator = detail::slot(alloc, at_accelerator);
      if (!value || !replicas || !accelerator) return py::none();
      double v = 0.0;
      int64_t r = 0, type = -1, u = 0;
      if (!detail::exact_double(value, &v) || !detail::exact_int64(replicas, &r) ||
          !PyUnicode_CheckExact(accelerator))
        return py::none();
      if (PyObject *t = detail::lookup(types.ptr(), accelerator)) {
        if (!detail::exact_int64(t, &type) || type < 0 || type >= n_types) return py::none();
        // a pair the model has no instance count for takes 0 units, as
        // Model.get_num_instances answers
        if (PyObject *pair = detail::lookup(model_units, accelerator))
          if (!detail::exact_int64(pair, &u)) return py::none();
      }
      if (!b.add(v, r, (int32_t)type, u)) return py::none();
      if (PyList_Append(candidates.ptr(), alloc) != 0) throw py::error_already_set();
    }
    if (b.allocations() - b.alloc_offset.back() != PyDict_GET_SIZE(allocs.ptr())) return py::none();
    b.end_server(prio);
  }

  const Problem p = b.problem(capacity_data, (int)n_types, delayed_best_effort, policy);
  if (const char *what = check(p)) throw std::invalid_argument(what);
  std::vector<int32_t> chosen((size_t)n_servers);
  std::vector<int64_t> granted((size_t)n_servers);
  solve(p, chosen.data(), granted.data());

  py::list chosen_out((size_t)n_servers), granted_out((size_t)n_servers),
      offsets_out((size_t)n_servers + 1);
  for (py::ssize_t s = 0; s < n_servers; ++s) {
    chosen_out[(size_t)s] = py::int_((long long)chosen[(size_t)s]);
    granted_out[(size_t)s] = py::int_((long long)granted[(size_t)s]);
  }
  for (py::ssize_t s = 0; s <= n_servers; ++s)
    offsets_out[(size_t)s] = py::int_((long long)b.alloc_offset[(size_t)s]);
  return py::make_tuple(chosen_out, granted_out, candidates, offsets_out);
}

inline void bind(py::module_ &m) {
  m.def("greedy_solve", &greedy_solve,
        "Limited-mode greedy solve over flat arrays (greedy_core.h); returns "
        "(chosen index per server or -1, granted replicas per server)",
        py::arg("capacity"), py::arg("priority"), py::arg("alloc_offset"), py::arg("value"),
        py::arg("num_replicas"), py::arg("type_index"), py::arg("units_per_replica"),
        py::arg("delayed_best_effort"), py::arg("policy"));
  m.attr("HAS_GREEDY") = true;
  m.def("greedy_solve_objects", &greedy_solve_objects,
        "The same solve with value, num_replicas and accelerator read from the "
        "servers' all_allocations; returns (chosen, granted, every candidate in "
        "order, their offsets per server), or None when the array route has to "
        "decide",
        py::arg("servers"), py::arg("priority"), py::arg("capacity"), py::arg("types"),
        py::arg("units"), py::arg("allocation_type"), py::arg("delayed_best_effort"),
        py::arg("policy"));
  m.attr("HAS_GREEDY_OBJECTS") = true;
}

}  // namespace greedy
}  // namespace wva
