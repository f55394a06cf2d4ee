// runs_epoch_test.cpp — the look-back epoch accounting of the one-launch packed recover
// (csrc/fec_forms.hpp runs_epochs, called by fec_shim.cpp runs_workspace) driven through long
// call sequences on the CPU: a workspace's counter as the shim keeps it, calls of 1..64 launches
// drawn at random, at the real limit (2^30, counter started just below it) and at small ones
// that wrap every few calls.  Checked per call, against a model that restates the rule:
//   1. every epoch handed out is non-zero and below min(limit, 2^30): it fits the 30 bits above
//      kRunEpochShift, and a zeroed look-back word (epoch 0) never matches;
//   2. the epochs of one call are consecutive: first .. first + n - 1;
//   3. no epoch is handed out twice between two re-zeroes of the workspace;
//   4. a re-zero is asked for exactly when last + n >= limit (last: the last epoch used since
//      the workspace was zeroed, 0 for none).
// Prints "OK <calls> calls <re-zeroes> re-zeroes" or the first violation, and exits non-zero.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/runs_epoch_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_set>

#include "fec_forms.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_random() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Totals {
  uint64_t calls = 0, rezeroes = 0;
};

[[noreturn]] void fail(const char* what, uint32_t limit, uint64_t call, uint32_t last, uint32_t n, uint32_t first) {
  std::printf("FAIL %s: limit=%u call=%llu last=%u n=%u first=%u\n", what, limit, static_cast<unsigned long long>(call),
              last, n, first);
  std::exit(1);
}

// One workspace's life: `calls` calls from a counter that starts at `start` (as if earlier calls
// had used epochs 1..start since the workspace was zeroed).
void run(uint32_t limit, uint32_t start, uint64_t calls, uint32_t max_n, Totals& tot) {
  constexpr uint64_t kEpochBits = 1ull << 30;      // what fits above kRunEpochShift = 34 in 64 bits
  std::unordered_set<uint32_t> used;               // epochs handed out since the last re-zero
  uint32_t counter = start;                        // the shim's StreamWorkspace::epoch
  uint64_t model_last = start;                     // the model's own count, kept apart from it
  bool wrapped = false;                            // epochs 1..start are in use until the first re-zero
  for (uint64_t c = 0; c < calls; ++c) {
    const uint32_t n = 1 + static_cast<uint32_t>(next_random() % max_n);
    const qfec::RunsEpochs e = qfec::runs_epochs(counter, n, limit);
    const bool want_rezero = model_last + n >= limit;
    if (e.rezero != want_rezero) fail("re-zero not as the rule says", limit, c, counter, n, e.first);
    if (e.rezero) {
      used.clear();
      model_last = 0;
      wrapped = true;
      ++tot.rezeroes;
    }
    if (e.first != model_last + 1) fail("epochs not consecutive with the last one used", limit, c, counter, n, e.first);
    for (uint32_t i = 0; i < n; ++i) {             // the launcher passes epoch + c to launch c
      const uint64_t ep = static_cast<uint64_t>(e.first) + i;
      if (ep == 0 || ep >= limit || ep >= kEpochBits) fail("epoch out of range", limit, c, counter, n, e.first);
      if (!wrapped && ep <= start) fail("epoch of the workspace's earlier life handed out again", limit, c, counter, n, e.first);
      if (!used.insert(static_cast<uint32_t>(ep)).second) fail("epoch handed out twice", limit, c, counter, n, e.first);
    }
    counter = e.first + n - 1;                     // what runs_workspace stores back
    model_last += n;
    ++tot.calls;
  }
}

}  // namespace

int main() {
  static_assert(qfec::kRunsEpochLimit == 1u << 30, "30 bits of epoch above kRunEpochShift");
  Totals tot;
  // the real limit: from zero (no wrap in sight), and from just below 2^30 (wraps within a few calls)
  run(qfec::kRunsEpochLimit, 0, 20000, 64, tot);
  const uint64_t before = tot.rezeroes;
  if (before != 0) fail("re-zero far from the limit", qfec::kRunsEpochLimit, 0, 0, 0, 0);
  for (uint32_t below = 1; below <= 200; ++below) run(qfec::kRunsEpochLimit, qfec::kRunsEpochLimit - below, 300, 64, tot);
  if (tot.rezeroes - before != 200) fail("one wrap per run that starts below the limit", qfec::kRunsEpochLimit, 0, 0, 0, 0);
  // small limits: every call count n < limit, wraps every few calls
  for (uint32_t limit : {2u, 3u, 16u, 17u, 65u, 66u, 100u, 1000u, 4097u}) {
    const uint32_t max_n = limit - 1 < 64 ? limit - 1 : 64;
    for (uint32_t start : {0u, 1u, limit / 2, limit - 1})
      if (start < limit) run(limit, start, 50000, max_n, tot);
  }
  std::printf("OK %llu calls %llu re-zeroes\n", static_cast<unsigned long long>(tot.calls),
              static_cast<unsigned long long>(tot.rezeroes));
  return 0;
}
