// Laying a fleet out as a greedy::Problem one allocation at a time: plain
// C++17, no Python, no torch, no HIP.  greedy_py.h walks the servers'
// Allocation objects and feeds what it reads to a Builder; the Builder keeps
// the offsets, applies the bounds of wva_amd/solver/greedy.py and owns the
// arrays the Problem points into (docs/design/native-greedy.md).
//
// A Builder refuses (add returns false, and the caller takes another route)
// whatever greedy.py's _marshal might refuse.  It may refuse more, never
// less: the value rule here is "every value finite and the sum of their
// magnitudes at most kMaxValueSum", which implies a finite sum in any order
// and under any summation scheme.

#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "greedy_core.h"

namespace wva {
namespace greedy {

// greedy.py: _MAX_REPLICAS, _MAX_UNITS, _MAX_ALLOCATIONS
constexpr int64_t kMaxReplicas = int64_t(1) << 31;
constexpr int64_t kMaxUnits = int64_t(1) << 12;
constexpr int64_t kMaxAllocations = int64_t(1) << 18;
constexpr double kMaxValueSum = 1e300;

struct Builder {
  std::vector<int64_t> priority;      // [servers]
  std::vector<int64_t> alloc_offset;  // [servers + 1]
  std::vector<double> value;          // [allocations] ...
  std::vector<int64_t> num_replicas;
  std::vector<int32_t> type_index;
  std::vector<int64_t> units_per_replica;
  double magnitude = 0.0;  // sum of |value|

  Builder() : alloc_offset(1, 0) {}

  void reserve(size_t servers, size_t allocations) {
    priority.reserve(servers);
    alloc_offset.reserve(servers + 1);
    value.reserve(allocations);
    num_replicas.reserve(allocations);
    type_index.reserve(allocations);
    units_per_replica.reserve(allocations);
  }

  int64_t allocations() const { return (int64_t)value.size(); }

  // One allocation of the server that end_server() will close.  type < 0 is
  // an accelerator the system does not know; its units are stored as 0.
  // false: out of the bounds, nothing was added.
  bool add(double v, int64_t replicas, int32_t type, int64_t units) {
    if (!std::isfinite(v)) return false;
    const double sum = magnitude + std::fabs(v);
    if (!(sum <= kMaxValueSum)) return false;
    if (replicas <= -kMaxReplicas || replicas >= kMaxReplicas) return false;
    if (type < 0) {
      type = -1;
      units = 0;
    }
    if (units <= -kMaxUnits || units >= kMaxUnits) return false;
    if (allocations() + 1 >= kMaxAllocations) return false;
    magnitude = sum;
    value.push_back(v);
    num_replicas.push_back(replicas);
    type_index.push_back(type);
    units_per_replica.push_back(units);
    return true;
  }

  void end_server(int64_t server_priority) {
    priority.push_back(server_priority);
    alloc_offset.push_back(allocations());
  }

  // The Problem over this Builder's arrays; valid while the Builder lives
  // and is not added to.
  Problem problem(const int64_t *capacity, int n_types, bool delayed_best_effort,
                  int policy) const {
    Problem p;
    p.n_types = n_types;
    p.capacity = capacity;
    p.n_servers = (int)priority.size();
    p.priority = priority.data();
    p.alloc_offset = alloc_offset.data();
    p.value = value.data();
    p.num_replicas = num_replicas.data();
    p.type_index = type_index.data();
    p.units_per_replica = units_per_replica.data();
    p.delayed_best_effort = delayed_best_effort;
    p.policy = policy;
    return p;
  }
};

}  // namespace greedy
}  // namespace wva
