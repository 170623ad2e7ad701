// Limited-mode greedy solve over flat arrays: plain C++17, no Python, no
// torch, no HIP.  A port of wva_amd/solver/greedy.py, which stays the
// reference it is held to (tests/test_greedy_native.py); the layout and
// the fallback rules are in docs/design/native-greedy.md.
//
// Servers come in system.servers order; server s owns the allocations
// [alloc_offset[s], alloc_offset[s + 1]) in the order of
// server.all_allocations.values().  Per allocation: value, num_replicas,
// type_index (index into capacity[], -1 for an accelerator the system does
// not know) and units_per_replica (instances * multiplicity).  The result is,
// per server, the index of the chosen allocation within its slice (-1: none)
// and the granted replica count.
//
// The only floating-point operation is the subtraction that forms a regret
// delta; everything else on doubles is a comparison.  Rescaling cost and
// value of a partially granted allocation is left to the caller, so the
// results cannot differ from the Python solve by a bit.  Build without
// -ffast-math.
//
// The caller guarantees finite values and integers small enough that
// sum |capacity| + sum |num_replicas * units_per_replica| fits int64.

#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace wva {
namespace greedy {

enum Policy : int {
  kNone = 0,
  kPriorityExhaustive = 1,
  kPriorityRoundRobin = 2,
  kRoundRobin = 3,
};

struct Problem {
  int n_types = 0;
  const int64_t *capacity = nullptr;  // [n_types]
  int n_servers = 0;
  const int64_t *priority = nullptr;      // [n_servers]
  const int64_t *alloc_offset = nullptr;  // [n_servers + 1]
  const double *value = nullptr;          // [alloc_offset[n_servers]] ...
  const int64_t *num_replicas = nullptr;
  const int32_t *type_index = nullptr;
  const int64_t *units_per_replica = nullptr;
  bool delayed_best_effort = false;
  int policy = kNone;
};

// nullptr when the arrays are consistent, else what is wrong with them
inline const char *check(const Problem &p) {
  if (p.n_types < 0 || p.n_servers < 0) return "negative length";
  if (p.policy < kNone || p.policy > kRoundRobin) return "unknown policy";
  if (p.alloc_offset[0] != 0) return "alloc_offset[0] must be 0";
  for (int s = 0; s < p.n_servers; ++s)
    if (p.alloc_offset[s + 1] < p.alloc_offset[s]) return "alloc_offset must not decrease";
  const int64_t n = p.alloc_offset[p.n_servers];
  for (int64_t i = 0; i < n; ++i)
    if (p.type_index[i] < -1 || p.type_index[i] >= p.n_types) return "type_index out of range";
  return nullptr;
}

namespace detail {

// one server with at least one allocation (greedy.py: ServerEntry)
struct Entry {
  int server;
  int64_t priority;
  int64_t first;  // into Solver::sorted
  int64_t count;
  int64_t cur;
  double delta;
};

// floor division for b > 0, as Python's //
inline int64_t floor_div(int64_t a, int64_t b) {
  int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

struct Solver {
  const Problem &p;
  int32_t *chosen;
  int64_t *granted;
  std::vector<int64_t> available;
  std::vector<int64_t> sorted;  // global allocation indices, per server by value
  std::vector<Entry> entries;

  Solver(const Problem &problem, int32_t *chosen_out, int64_t *granted_out)
      : p(problem), chosen(chosen_out), granted(granted_out),
        available(problem.capacity, problem.capacity + problem.n_types) {}

  int64_t alloc_of(const Entry &e, int64_t k) const { return sorted[(size_t)(e.first + k)]; }
  double cur_value(const Entry &e) const { return p.value[alloc_of(e, e.cur)]; }

  void grant(const Entry &e, int64_t alloc, int64_t replicas) {
    chosen[e.server] = (int32_t)(alloc - p.alloc_offset[e.server]);
    granted[e.server] = replicas;
  }

  // _order_cmp: priority ascending, delta descending, current value descending
  int order_cmp(const Entry &a, const Entry &b) const {
    if (a.priority != b.priority) return a.priority < b.priority ? -1 : 1;
    if (a.delta != b.delta) return b.delta < a.delta ? -1 : 1;
    const double av = cur_value(a), bv = cur_value(b);
    if (av == bv) return 0;
    return bv < av ? -1 : 1;
  }

  void build_entries() {
    const int64_t n = p.alloc_offset[p.n_servers];
    sorted.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) sorted[(size_t)i] = i;
    entries.reserve((size_t)p.n_servers);
    for (int s = 0; s < p.n_servers; ++s) {
      const int64_t first = p.alloc_offset[s], count = p.alloc_offset[s + 1] - first;
      if (count == 0) continue;
      std::stable_sort(sorted.begin() + first, sorted.begin() + first + count,
                       [this](int64_t a, int64_t b) { return p.value[a] < p.value[b]; });
      Entry e{s, p.priority[s], first, count, 0, std::numeric_limits<double>::infinity()};
      if (count > 1) e.delta = p.value[alloc_of(e, 1)] - p.value[alloc_of(e, 0)];
      entries.push_back(e);
    }
    // the key (priority, -delta, -value), stable
    std::stable_sort(entries.begin(), entries.end(), [this](const Entry &a, const Entry &b) {
      if (a.priority != b.priority) return a.priority < b.priority;
      if (a.delta != b.delta) return a.delta > b.delta;
      return cur_value(a) > cur_value(b);
    });
  }

  // _allocate over entries[order[*]]; appends what ran off its last
  // allocation to unallocated
  void allocate(std::vector<int> order, std::vector<int> &unallocated) {
    size_t head = 0;
    while (head < order.size()) {
      Entry &top = entries[(size_t)order[head++]];
      const int64_t alloc = alloc_of(top, top.cur);
      const int32_t type = p.type_index[alloc];
      if (type < 0) continue;  // unknown accelerator: the entry vanishes
      const int64_t count = p.num_replicas[alloc] * p.units_per_replica[alloc];
      if (available[(size_t)type] >= count) {
        available[(size_t)type] -= count;
        grant(top, alloc, p.num_replicas[alloc]);
        continue;
      }
      top.cur += 1;
      if (top.cur + 1 < top.count) {
        top.delta = p.value[alloc_of(top, top.cur + 1)] - p.value[alloc_of(top, top.cur)];
      } else if (top.cur == top.count) {
        unallocated.push_back((int)(&top - entries.data()));
        continue;
      } else {
        top.delta = std::numeric_limits<double>::infinity();
      }
      // _insort: leftmost i with cmp(entries[i], top) >= 0
      size_t lo = head, hi = order.size();
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (order_cmp(entries[(size_t)order[mid]], top) < 0)
          lo = mid + 1;
        else
          hi = mid;
      }
      order.insert(order.begin() + (std::ptrdiff_t)lo, (int)(&top - entries.data()));
    }
  }

  // _allocate_maximally: one server at a time, as much as fits
  void allocate_maximally(const std::vector<int> &group) {
    for (int idx : group) {
      const Entry &e = entries[(size_t)idx];
      for (int64_t k = 0; k < e.count; ++k) {
        const int64_t alloc = alloc_of(e, k);
        const int32_t type = p.type_index[alloc];
        const int64_t units = p.units_per_replica[alloc];
        if (type < 0 || units <= 0) continue;
        const int64_t replicas =
            std::min(floor_div(available[(size_t)type], units), p.num_replicas[alloc]);
        if (replicas > 0) {
          grant(e, alloc, replicas);
          available[(size_t)type] -= replicas * units;
          break;
        }
      }
    }
  }

  // _allocate_equally: one replica per visit until nothing more fits
  void allocate_equally(const std::vector<int> &group) {
    struct Ticket {
      bool live = true, active = false;
      int32_t type = -1;
      int64_t units = 0, alloc = -1, replicas = 0;
    };
    std::vector<Ticket> tickets(group.size());
    size_t live = group.size();
    while (live > 0) {
      for (size_t g = 0; g < group.size(); ++g) {
        Ticket &t = tickets[g];
        if (!t.live) continue;
        const Entry &e = entries[(size_t)group[g]];
        if (!t.active) {
          for (int64_t k = 0; k < e.count; ++k) {
            const int64_t alloc = alloc_of(e, k);
            const int32_t type = p.type_index[alloc];
            if (type < 0) continue;
            const int64_t units = p.units_per_replica[alloc];
            if (units > 0 && available[(size_t)type] >= units) {
              t.active = true;
              t.type = type;
              t.units = units;
              t.alloc = alloc;
              break;
            }
          }
          if (!t.active) {
            t.live = false;
            --live;
            continue;
          }
        }
        const int64_t fit = floor_div(available[(size_t)t.type], t.units);
        if (std::min(fit, p.num_replicas[t.alloc]) > 0) {
          t.replicas += 1;
          available[(size_t)t.type] -= t.units;
        } else {
          t.live = false;
          --live;
        }
      }
    }
    for (size_t g = 0; g < group.size(); ++g)
      if (tickets[g].replicas > 0) grant(entries[(size_t)group[g]], tickets[g].alloc, tickets[g].replicas);
  }

  // make_priority_groups: runs of equal priority
  std::vector<std::vector<int>> priority_groups(const std::vector<int> &order) const {
    std::vector<std::vector<int>> groups;
    for (size_t i = 0; i < order.size(); ++i) {
      if (i == 0 || entries[(size_t)order[i]].priority != entries[(size_t)order[i - 1]].priority)
        groups.emplace_back();
      groups.back().push_back(order[i]);
    }
    return groups;
  }

  void best_effort(const std::vector<int> &unallocated) {
    switch (p.policy) {
      case kPriorityExhaustive:
        allocate_maximally(unallocated);
        break;
      case kPriorityRoundRobin:
        for (const auto &group : priority_groups(unallocated)) allocate_equally(group);
        break;
      case kRoundRobin:
        allocate_equally(unallocated);
        break;
      default:
        break;  // kNone: nothing beyond satisfying SLOs
    }
  }

  void run() {
    for (int s = 0; s < p.n_servers; ++s) {
      chosen[s] = -1;
      granted[s] = 0;
    }
    build_entries();
    std::vector<int> all(entries.size());
    for (size_t i = 0; i < all.size(); ++i) all[i] = (int)i;
    if (p.delayed_best_effort) {
      std::vector<int> unallocated;
      allocate(all, unallocated);
      best_effort(unallocated);
    } else {
      for (const auto &group : priority_groups(all)) {
        std::vector<int> unallocated;
        allocate(group, unallocated);
        best_effort(unallocated);
      }
    }
  }
};

}  // namespace detail

// chosen[n_servers], granted[n_servers]; available_out (optional,
// [n_types]) receives what is left of the capacity.  p must pass check().
inline void solve(const Problem &p, int32_t *chosen, int64_t *granted,
                  int64_t *available_out = nullptr) {
  detail::Solver solver(p, chosen, granted);
  solver.run();
  if (available_out) std::copy(solver.available.begin(), solver.available.end(), available_out);
}

}  // namespace greedy
}  // namespace wva
