"""csrc/greedy_core.h under AddressSanitizer and UBSan, as a stand-alone program.

The header is plain C++17, so it is checked where sanitizers belong: in a
small program with its own ``main``, built with
``g++ -std=c++17 -fsanitize=address,undefined`` and run as a child process.
Nothing is loaded into Python under a sanitizer.  The program draws seeded
random inputs of the shapes tests/test_greedy_native.py uses (1-12 servers,
0-4 allocations each, few distinct values, three priority levels, units from
{1, 2, 4, 8}, small capacities with zeros, unknown accelerators), runs all
four policies with best effort delayed or not, and checks that

- what is left of every capacity is never negative (the inputs are not),
  and equals the capacity minus what the granted allocations take;
- every chosen index lies in its server's slice, and is -1 for a server
  without allocations;
- granted replicas are at most the requested ones.

CPU only; never part of a GPU run.
"""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "wva_amd" / "csrc"

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "greedy_core.h"

int main() {
  std::mt19937_64 rng(20260);
  auto pick = [&rng](int n) { return (int)(rng() % (uint64_t)n); };
  const double values[] = {0.0, 1.0, 2.0, 3.0, 5.0};
  const int64_t replicas[] = {0, 1, 1, 2, 3, 4, 6};
  const int64_t capacities[] = {0, 0, 1, 2, 4, 8, 12, 16, 32, 64};
  const int64_t units[] = {1, 2, 4, 8};
  long solves = 0, granted_total = 0, partial = 0, unallocated = 0;
  for (int round = 0; round < 4000; ++round) {
    const int n_types = 1 + pick(3);
    std::vector<int64_t> capacity((size_t)n_types);
    for (auto &c : capacity) c = capacities[pick(10)];
    const int n_servers = round == 0 ? 0 : 1 + pick(12);
    std::vector<int64_t> priority, offset{0}, reps, upr;
    std::vector<double> value;
    std::vector<int32_t> type;
    for (int s = 0; s < n_servers; ++s) {
      priority.push_back(1 + pick(3));
      const int n = pick(5);
      for (int k = 0; k < n; ++k) {
        value.push_back(values[pick(5)]);
        reps.push_back(replicas[pick(7)]);
        type.push_back(pick(20) == 0 ? -1 : pick(n_types));
        upr.push_back(type.back() < 0 ? 0 : units[pick(4)] * units[pick(4)]);
      }
      offset.push_back((int64_t)value.size());
    }
    for (int policy = 0; policy < 4; ++policy) {
      for (int delayed = 0; delayed < 2; ++delayed) {
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
        if (const char *what = wva::greedy::check(p)) {
          std::printf("FAIL round %d: check says %s\n", round, what);
          return 1;
        }
        std::vector<int32_t> chosen((size_t)n_servers, 77);
        std::vector<int64_t> granted((size_t)n_servers, 77);
        std::vector<int64_t> left((size_t)n_types, -77);
        wva::greedy::solve(p, chosen.data(), granted.data(), left.data());
        ++solves;
        std::vector<int64_t> expect(capacity);
        for (int s = 0; s < n_servers; ++s) {
          const int64_t n = offset[(size_t)s + 1] - offset[(size_t)s];
          if (chosen[(size_t)s] < -1 || chosen[(size_t)s] >= n) {
            std::printf("FAIL round %d server %d: index %d of %lld\n", round, s,
                        (int)chosen[(size_t)s], (long long)n);
            return 1;
          }
          if (chosen[(size_t)s] < 0) {
            if (granted[(size_t)s] != 0) {
              std::printf("FAIL round %d server %d: replicas without an allocation\n", round, s);
              return 1;
            }
            unallocated += n > 0;
            continue;
          }
          const size_t a = (size_t)(offset[(size_t)s] + chosen[(size_t)s]);
          if (granted[(size_t)s] > reps[a] || granted[(size_t)s] < 0 || type[a] < 0) {
            std::printf("FAIL round %d server %d: granted %lld of %lld, type %d\n", round, s,
                        (long long)granted[(size_t)s], (long long)reps[a], (int)type[a]);
            return 1;
          }
          partial += granted[(size_t)s] < reps[a];
          granted_total += granted[(size_t)s];
          expect[(size_t)type[a]] -= granted[(size_t)s] * upr[a];
        }
        for (int t = 0; t < n_types; ++t) {
          if (left[(size_t)t] < 0 || left[(size_t)t] != expect[(size_t)t]) {
            std::printf("FAIL round %d type %d: %lld left, expected %lld\n", round, t,
                        (long long)left[(size_t)t], (long long)expect[(size_t)t]);
            return 1;
          }
        }
      }
    }
  }
  if (granted_total == 0 || partial == 0 || unallocated == 0) {
    std::printf("FAIL: the inputs never granted, never granted in part or never refused\n");
    return 1;
  }
  std::printf("OK %ld solves, %ld replicas granted, %ld partial grants, %ld servers refused\n",
              solves, granted_total, partial, unallocated);
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


def test_greedy_core_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None or not sanitizer_runtime_present(gxx, tmp_path):
        pytest.skip("g++ with the address and undefined-behaviour sanitizer runtimes is not here")
    source = tmp_path / "greedy_sanitized.cpp"
    source.write_text(PROGRAM)
    program = tmp_path / "greedy_sanitized"
    built = subprocess.run(
        [gxx, *FLAGS, "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(source), "-o", str(program)],
        capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("OK "), ran.stdout
    assert not ran.stderr, ran.stderr
