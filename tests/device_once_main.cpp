// Stand-alone host program for DeviceOnce, the bookkeeping half of sam_pt_amd/csrc/dyn_lds.h (no HIP header, no GPU):
// test_cpu_host.py builds it with the host compiler under -fsanitize=thread and runs it.  Exit status 0 = every assertion held.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../sam_pt_amd/csrc/dyn_lds.h"

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

int main() {
  constexpr int THREADS = 8, ORDINALS = 4, ROUNDS = 2000, FLAKY = 2;
  sampt::DeviceOnce once;
  std::atomic<int> calls[ORDINALS] = {}, ok[ORDINALS] = {};
  int plain[ORDINALS] = {};            // written by the callable without any lock of its own: the class has to serialise it
  std::atomic<bool> go{false};
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; ++t)
    pool.emplace_back([&, t] {
      while (!go.load()) std::this_thread::yield();
      for (int i = 0; i < ROUNDS; ++i) {
        const int d = (t + i) % ORDINALS;
        const int rc = once.run(d, [&] {
          const int n = calls[d].fetch_add(1);
          if (d == FLAKY && n == 0) return 7;      // this ordinal's first attempt fails: not remembered
          ++plain[d];
          ok[d].fetch_add(1);
          return 0;
        });
        REQUIRE(rc == 0 || (d == FLAKY && rc == 7));
      }
    });
  go.store(true);
  for (auto& th : pool) th.join();
  for (int d = 0; d < ORDINALS; ++d) {
    REQUIRE(ok[d].load() == 1 && plain[d] == 1);                 // succeeded exactly once per ordinal
    REQUIRE(calls[d].load() == (d == FLAKY ? 2 : 1));            // the failed first call was tried again, once
  }
  int outside = 0;
  for (int i = 0; i < 5; ++i) {                                  // ordinals beyond the table: every time
    REQUIRE(once.run(sampt::DeviceOnce::MAX_DEVICES, [&] { return ++outside, 0; }) == 0);
    REQUIRE(once.run(-1, [&] { return ++outside, 0; }) == 0);
  }
  REQUIRE(outside == 10);
  REQUIRE(once.run(sampt::DeviceOnce::MAX_DEVICES - 1, [&] { return ++outside, 0; }) == 0);   // the last one inside: once
  REQUIRE(once.run(sampt::DeviceOnce::MAX_DEVICES - 1, [&] { return ++outside, 0; }) == 0);
  REQUIRE(outside == 11);
  std::puts("device_once: ok");
  return 0;
}
