"""csrc/greedy_objects.h under AddressSanitizer and UBSan, as a stand-alone program.

The header is plain C++17 (the Builder that greedy_py.h fills while it walks
the servers' Allocation objects), so it is checked the way
tests/test_greedy_native_sanitized.py checks greedy_core.h: in a small program
with its own ``main``, built with ``g++ -std=c++17
-fsanitize=address,undefined`` and run as a child process.  Nothing is loaded
into Python under a sanitizer.  The program

- feeds seeded random fleets (the shapes of tests/test_greedy_native.py,
  servers without allocations included) to a Builder one allocation at a
  time, next to plain vectors filled directly, and requires equal arrays,
  a Problem that passes ``check`` and equal solves from both, under all four
  policies with best effort delayed or not;
- requires an unknown accelerator (type < 0) to be stored as type -1 with 0
  units whatever units came with it;
- requires ``add`` to refuse, and to leave the Builder as it was, for a NaN,
  an infinity, a magnitude sum beyond the bound, replicas at +-2**31, units
  at +-2**12 and the 2**18th allocation, and to take the values just inside.

CPU only; never part of a GPU run.
"""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "wva_amd" / "csrc"

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "greedy_objects.h"

using wva::greedy::Builder;

#define REQUIRE(cond)                                              \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);          \
      return 1;                                                    \
    }                                                              \
  } while (0)

int bounds() {
  const double inf = std::numeric_limits<double>::infinity();
  Builder b;
  REQUIRE(b.add(1.0, 3, 0, 2));
  const int64_t before = b.allocations();
  REQUIRE(!b.add(std::nan(""), 1, 0, 1));
  REQUIRE(!b.add(inf, 1, 0, 1));
  REQUIRE(!b.add(-inf, 1, 0, 1));
  REQUIRE(!b.add(1.0, int64_t(1) << 31, 0, 1));
  REQUIRE(!b.add(1.0, -(int64_t(1) << 31), 0, 1));
  REQUIRE(!b.add(1.0, 1, 0, int64_t(1) << 12));
  REQUIRE(!b.add(1.0, 1, 0, -(int64_t(1) << 12)));
  REQUIRE(!b.add(1.1e300, 1, 0, 1));
  REQUIRE(b.allocations() == before && b.magnitude == 1.0);
  REQUIRE(b.add(1.0, (int64_t(1) << 31) - 1, 0, (int64_t(1) << 12) - 1));
  REQUIRE(b.add(-2.0, -(int64_t(1) << 31) + 1, 0, -(int64_t(1) << 12) + 1));
  REQUIRE(b.magnitude == 4.0);
  // an unknown accelerator keeps no units, and its units are not a reason to refuse
  REQUIRE(b.add(0.5, 1, -7, int64_t(1) << 40));
  REQUIRE(b.type_index.back() == -1 && b.units_per_replica.back() == 0);
  // magnitudes add up whatever the signs
  REQUIRE(b.add(6e299, 1, 0, 1));
  REQUIRE(!b.add(-6e299, 1, 0, 1));
  b.end_server(1);
  REQUIRE(b.alloc_offset.size() == 2 && b.alloc_offset[1] == b.allocations());

  Builder many;
  for (int64_t i = 0; i + 1 < wva::greedy::kMaxAllocations; ++i) REQUIRE(many.add(0.0, 1, 0, 1));
  REQUIRE(many.allocations() == wva::greedy::kMaxAllocations - 1);
  REQUIRE(!many.add(0.0, 1, 0, 1));
  REQUIRE(many.allocations() == wva::greedy::kMaxAllocations - 1);
  return 0;
}

int main() {
  if (bounds() != 0) return 1;
  std::mt19937_64 rng(20261);
  auto pick = [&rng](int n) { return (int)(rng() % (uint64_t)n); };
  const double values[] = {0.0, 1.0, 2.0, 3.0, 5.0};
  const int64_t replicas[] = {0, 1, 1, 2, 3, 4, 6};
  const int64_t capacities[] = {0, 0, 1, 2, 4, 8, 12, 16, 32, 64};
  const int64_t units[] = {1, 2, 4, 8};
  long solves = 0, granted_total = 0, empty_servers = 0, unknown = 0;
  for (int round = 0; round < 2000; ++round) {
    const int n_types = 1 + pick(3);
    std::vector<int64_t> capacity((size_t)n_types);
    for (auto &c : capacity) c = capacities[pick(10)];
    const int n_servers = round == 0 ? 0 : 1 + pick(12);
    std::vector<int64_t> priority, offset{0}, reps, upr;
    std::vector<double> value;
    std::vector<int32_t> type;
    Builder b;
    if (round % 2) b.reserve((size_t)n_servers, 8);
    for (int s = 0; s < n_servers; ++s) {
      const int64_t prio = 1 + pick(3);
      const int n = pick(5);
      empty_servers += n == 0;
      for (int k = 0; k < n; ++k) {
        const bool known = pick(20) != 0;
        unknown += !known;
        const int32_t t = known ? pick(n_types) : -1 - pick(3);
        const int64_t u = units[pick(4)] * units[pick(4)];
        value.push_back(values[pick(5)]);
        reps.push_back(replicas[pick(7)]);
        type.push_back(known ? t : -1);
        upr.push_back(known ? u : 0);
        REQUIRE(b.add(value.back(), reps.back(), t, u));
      }
      priority.push_back(prio);
      offset.push_back((int64_t)value.size());
      b.end_server(prio);
    }
    REQUIRE(b.priority == priority && b.alloc_offset == offset && b.value == value);
    REQUIRE(b.num_replicas == reps && b.type_index == type && b.units_per_replica == upr);
    for (int policy = 0; policy < 4; ++policy) {
      for (int delayed = 0; delayed < 2; ++delayed) {
        const wva::greedy::Problem built = b.problem(capacity.data(), n_types, delayed != 0, policy);
        REQUIRE(built.n_servers == n_servers && built.n_types == n_types);
        REQUIRE(wva::greedy::check(built) == nullptr);
        wva::greedy::Problem p;
        p.n_types = n_types;
        p.capacity = capacity.data();
        p.n_servers = n_servers;
        p.priority = priority.data();
        p.alloc_offset = offset.data();
        p.value = value.data();
        p.num_replicas = reps.data();
        p.type_index = type.data();
        p.units_per_replica = upr.data();
        p.delayed_best_effort = delayed != 0;
        p.policy = policy;
        std::vector<int32_t> chosen((size_t)n_servers, 77), chosen_built((size_t)n_servers, 78);
        std::vector<int64_t> granted((size_t)n_servers, 77), granted_built((size_t)n_servers, 78);
        wva::greedy::solve(p, chosen.data(), granted.data());
        wva::greedy::solve(built, chosen_built.data(), granted_built.data());
        ++solves;
        REQUIRE(chosen == chosen_built && granted == granted_built);
        for (int s = 0; s < n_servers; ++s) granted_total += granted[(size_t)s];
      }
    }
  }
  REQUIRE(granted_total > 0 && empty_servers > 0 && unknown > 0);
  std::printf("OK %ld solves, %ld replicas granted, %ld servers without allocations, "
              "%ld unknown accelerators\n", solves, granted_total, empty_servers, unknown);
  return 0;
}
"""

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def sanitizer_runtime_present(gxx, tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run([gxx, *FLAGS, str(probe), "-o", str(tmp_path / "probe")],
                           capture_output=True, text=True)
    return built.returncode == 0


def test_greedy_objects_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None or not sanitizer_runtime_present(gxx, tmp_path):
        pytest.skip("g++ with the address and undefined-behaviour sanitizer runtimes is not here")
    source = tmp_path / "greedy_objects_sanitized.cpp"
    source.write_text(PROGRAM)
    program = tmp_path / "greedy_objects_sanitized"
    built = subprocess.run(
        [gxx, *FLAGS, "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(source), "-o", str(program)],
        capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("OK "), ran.stdout
    assert not ran.stderr, ran.stderr
