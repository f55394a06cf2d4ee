// fec_knobs.cpp — test and tuning switches (fec_knobs.hpp).  Compiled twice: plain for
// libfec_hip.so (every switch at its default, no environment read, no switch name in the
// library) and with -DQUICFEC_TEST_HOOKS for libfec_hip_test.so.
#include "fec_knobs.hpp"

#include <cstdlib>
#include <cstring>
#ifdef QUICFEC_TEST_HOOKS
#include <mutex>
#include <vector>
#endif

namespace qfec {

#ifdef QUICFEC_TEST_HOOKS

namespace {
const char* const kNames[] = {
    "QUICFEC_MAX_WAVE_BLOCKS",     "QUICFEC_MAX_LAUNCH_THREADS",   "QUICFEC_ENCODE_TILE",
    "QUICFEC_ENCODE_BLOCKS",       "QUICFEC_ENCODE_WAVES",         "QUICFEC_ENCODE_BITS",
    "QUICFEC_ENCODE_STAGE",        "QUICFEC_DECODE_WAVES",         "QUICFEC_ROWS_DIRECT_BLOCKS",
    "QUICFEC_RUNS_STAGE",          "QUICFEC_DECODE_SCAN",          "QUICFEC_PACKED_RUNS",
    "QUICFEC_RUNS_EPOCH_LIMIT",
    "QUICFEC_RESIDENT_TEST_NOLAUNCH", "QUICFEC_RESIDENT_TEST_EPOCH", "QUICFEC_RESIDENT_TEST_TEAR",
    "QUICFEC_RESIDENT_TEST_FAIL_AT", "QUICFEC_RESIDENT_SPREAD",    "QUICFEC_RESIDENT_STAMPS",
    "QUICFEC_RESIDENT_SLOW_US",    "QUICFEC_COALESCE_STAMPS",      "QUICFEC_COALESCE_SPIN_PAUSE",
    "QUICFEC_COALESCE_SPIN_YIELD",   "QUICFEC_PLAN_ARENA_BYTES",
};
static_assert(sizeof(kNames) / sizeof(kNames[0]) == static_cast<size_t>(TestKnob::kCount), "one name per switch");
}  // namespace

long test_knob(TestKnob k, long def) {
  const char* v = std::getenv(kNames[static_cast<int>(k)]);
  return v && *v ? std::atol(v) : def;
}

bool test_knobs_enabled() { return true; }

namespace {
std::mutex g_trace_mu;
std::vector<LaunchRecord> g_trace;  // at most kLaunchTraceCapacity records
uint64_t g_trace_seen = 0;          // launches since the last clear, kept or not
}  // namespace

void trace_launch(const LaunchRecord& rec) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  if (g_trace.size() < kLaunchTraceCapacity) g_trace.push_back(rec);
  ++g_trace_seen;
}

namespace {
uint64_t read_trace(int64_t* out, uint64_t max_records, int clear) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  const uint64_t seen = g_trace_seen;
  const uint64_t n = g_trace.size() < max_records ? g_trace.size() : max_records;
  if (out != nullptr && n > 0) std::memcpy(out, g_trace.data(), n * sizeof(LaunchRecord));
  if (clear) {
    g_trace.clear();
    g_trace_seen = 0;
  }
  return seen;
}
}  // namespace

#else

long test_knob(TestKnob, long def) { return def; }

bool test_knobs_enabled() { return false; }

void trace_launch(const LaunchRecord&) {}

namespace {
uint64_t read_trace(int64_t*, uint64_t, int) { return 0; }  // no trace in the product library
}  // namespace

#endif

}  // namespace qfec

// The trace's reader, exported by both libraries (they export the same C-ABI): copies up to
// max_records records of 16 int64 words (LaunchRecord) to `out` (nullable), oldest first,
// optionally clears the trace, and returns the launches seen since the last clear -- more than
// kLaunchTraceCapacity means the later ones were not kept.  libfec_hip.so keeps no trace: it
// writes nothing and returns 0.
extern "C" __attribute__((visibility("default"))) uint64_t fec_hip_launch_trace(int64_t* out, uint64_t max_records,
                                                                               int clear) {
  return qfec::read_trace(out, max_records, clear);
}
