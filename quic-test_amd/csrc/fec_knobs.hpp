// fec_knobs.hpp — the switches the library takes from the environment.
//
// Operational settings (the coalescer, the resident encoder's timings, host threads, the
// host-resident paths' thresholds; INTEGRATION.md §6 lists each with its default) are read by
// the product library where they are used.
//
// Test and tuning switches -- forcing a kernel form the library would not choose, sizes that
// make rare paths common (chunked launches, overflowing run images), fault injection into the
// resident encoder -- exist only in libfec_hip_test.so.  test_knob() is compiled twice
// (fec_knobs.cpp): in libfec_hip_test.so (-DQUICFEC_TEST_HOOKS) it reads the switch's
// environment variable at every call (tests change it inside one process); in libfec_hip.so it
// returns the default and no name of any such switch is in the library.  Both libraries are
// linked from the same kernel and shim objects.
#pragma once

#include <cstdint>

namespace qfec {

enum class TestKnob : int {
  kMaxWaveBlocks,     // workgroups per wave-per-group launch (forces the chunked launches)
  kMaxLaunchThreads,  // work items per launch of every other kernel (forces their chunked launches)
  kEncodeTile,        // groups per workgroup of the tiled encodes
  kEncodeBlocks,      // workgroups per CU of the tiled encodes
  kEncodeWaves,       // occupancy cap of the encodes, waves per CU
  kEncodeBits,        // 1: bit-sliced encode for every compiled shape, 0: never
  kEncodeStage,       // 1: parity rows staged through LDS, 0: direct stores
  kDecodeWaves,       // occupancy cap of the decodes, waves per CU
  kRowsDirectBlocks,  // block limit of the two-launch row prefix (forces the three-launch form)
  kRunsStage,         // run-image bytes of recover_runs (rows past it go straight to HBM)
  kDecodeScan,        // groups per wave of the mask-addressed decode
  kPackedRuns,        // 1: packed recover in one launch (recover_runs) whatever the loss, 0: never
  kRunsEpochLimit,    // look-back epochs of recover_runs before its workspace is re-zeroed (2^30)
  kResidentNoLaunch,  // resident encoder: record launches without launching (never serves)
  kResidentEpoch,     // resident encoder: tag epoch (short: scrubs within a few thousand calls)
  kResidentTear,      // resident encoder: store one chunk / later address words ~100 us late
  kResidentFailAt,    // resident encoder: this call (0 = first) fails as if its deadline passed
  kResidentSpread,    // resident encoder: every call to the next serving class
  kResidentStamps,    // resident encoder: phase time stamps of served batches, to stderr at exit
  kResidentSlowUs,    // resident encoder: slow-poll interval once idle
  kCoalesceStamps,    // coalescer: creation and first batches' phase times, to stderr
  kCoalesceSpinPause, // coalescer: a waiting caller's pause rounds before it yields
  kCoalesceSpinYield, // coalescer: ... and its yield rounds before it sleeps
  kPlanArenaBytes,    // record arena of a device-plan call, bytes (forces several plan chunks)
  kCount
};

// The switch from the environment, or `def` when unset; always `def` in libfec_hip.so.
long test_knob(TestKnob k, long def);

// Whether this library reads the test switches (libfec_hip_test.so).
bool test_knobs_enabled();

// ---- launch trace ----
// Every host launcher of the kernel translation units reports each kernel launch here, so that a test can
// see which kernel form produced the bytes it checks.  Like test_knob() this is compiled twice:
// in libfec_hip.so trace_launch() is an empty function and nothing is stored; in
// libfec_hip_test.so it appends the record to a bounded buffer (under a mutex: the batcher's
// flusher threads launch too).  Forms are numbers here; their names live with the reader's
// callers (quicfec.launch_trace), not in either library.
enum class LaunchForm : int64_t {
  kEncodeV16 = 1,
  kEncodeBits = 2,
  kEncodeBytes = 3,
  kClassify = 4,
  kDecodeFused = 5,
  kDecodeTiled = 6,
  kDecodeWave = 7,
  kDecodeBytes = 8,
  kRowsBlockSums = 9,
  kRowsScanBlocks = 10,
  kRowsWrite = 11,
  kRecoverRuns = 12,
  kFill = 13,
  kCopy = 14,
  kLegacyServer = 15,
  kDecodeV16 = 16,  // probe builds only
  kRunsRezero = 17,  // no kernel: recover_runs' workspace zeroed again because its epochs wrapped
};
// The address-table kernels (fec_gather.hip), numbered on from LaunchForm in a list of their own,
// as their forms are (fec_forms.hpp QFEC_TABLE_RECOVER_FORMS); named by quicfec.GATHER_LAUNCH_FORMS.
enum class GatherLaunchForm : int64_t {
  kClassifyGather = 18,
  kRecoverGather = 19,
};
// The variable-length address-table kernels (fec_gather_var.hip), numbered on in a list of their
// own again (fec_forms.hpp QFEC_TABLE_RECOVER_FORMS); named by quicfec.GATHER_VAR_LAUNCH_FORMS.
enum class GatherVarLaunchForm : int64_t {
  kClassifyGatherVar = 20,
  kRecoverGatherVar = 21,
  kEncodeGatherVar = 22,
};
// The scatter recover's kernels (fec_scatter.hip), numbered on in a list of their own
// (fec_forms.hpp QFEC_TABLE_RECOVER_FORMS); named by quicfec.SCATTER_LAUNCH_FORMS.
enum class ScatterLaunchForm : int64_t {
  kClassifyScatter = 23,
  kRecoverScatter = 24,  // LaunchRecord::first: 1 with a length table (VAR), 0 without
};
// The scatter encode's kernel (fec_scatter_encode.hip), numbered on in a list of its own
// (fec_forms.hpp QFEC_SCATTER_ENCODE_FORMS); named by quicfec.SCATTER_ENCODE_LAUNCH_FORMS.
enum class ScatterEncodeLaunchForm : int64_t {
  kEncodeScatter = 25,  // LaunchRecord::first: this pass owns the XOR row; LaunchRecord::direct: 1
                        // with a length table (VAR), 0 without
};

// The record builder of the device plans (fec_plan.hip), numbered on in a list of its own; named by
// quicfec.PLAN_LAUNCH_FORMS.
enum class PlanLaunchForm : int64_t {
  kBuildRecords = 26,  // first_item / items: the plan chunk's first group and its groups; aux: the
                       // arena slot of the launch's first group
};

// The kernels of the wide calls (fec_wide.hip), numbered on in a list of their own; named by
// quicfec.WIDE_LAUNCH_FORMS.
enum class WideLaunchForm : int64_t {
  kClassifyWide = 27,      // first_item / items: the launch's first group and its groups
  kBuildRecordsWide = 28,  // as kBuildRecords: the plan chunk's groups; aux: the arena slot of the first
  kDecodeWide = 29,        // first_item / items: groups of the call; k = 0, r = 8; pol; aux: first row of the pass
};

// The kernels of the wide address-table recover (fec_wide_table.hip), numbered on in a list of
// their own; named by quicfec.WIDE_TABLE_LAUNCH_FORMS.  Its record builds are kBuildRecordsWide's.
enum class WideTableLaunchForm : int64_t {
  kClassifyTableWide = 30,   // first_item / items: the launch's first group and its groups
  kRecoverScatterWide = 31,  // first_item / items: groups of the call; k = 0, r = 8; first: 1 with a
                             // length table (VAR), 0 without; pol; aux: first row of the pass
};

// The kernel of the wide scatter encode (fec_wide_encode.hip), numbered on in a list of its own;
// named by quicfec.WIDE_ENCODE_LAUNCH_FORMS.
enum class WideEncodeLaunchForm : int64_t {
  kEncodeScatterWide = 32,  // first_item / items: groups of the call; k = 0, r = 8; first: 1 with a
                            // length table (VAR), 0 without; pol; aux: first parity row of the pass
};

// One launch: 16 words, -1 where a field does not apply to the form.
struct LaunchRecord {
  int64_t form;          // LaunchForm
  int64_t k = -1;        // template K (0: the runtime-k instantiation)
  int64_t r = -1;        // template R (encodes, recover_runs) or MAXE (decodes)
  int64_t nm = -1;       // 16-B pieces per lane (decode_fused, recover_runs)
  int64_t nt = -1;       //  4-B pieces per lane
  int64_t off = -1;      // encode: OffsetKind of the instantiation
  int64_t first = -1;    // encode_v16: this pass owns the XOR row; recover_scatter: the length-table form
  int64_t pol = -1;      // memory policy / form bits (fec_forms.hpp kNtLoad .. kStageRows)
  int64_t direct = -1;   // decode_fused: mask-addressed; rows_write: writes the total itself;
                         // encode_scatter: the length-table form
  int64_t scan = -1;     // decode_fused: groups per wave of the scan form (0: one wave per group)
  int64_t tile = -1;     // groups per workgroup of the tiled mappings, 0 = flat mapping
  int64_t grid = 0;      // workgroups
  int64_t block = 0;     // work items per workgroup
  int64_t first_item = 0;  // first group (fill / copy: first 16-B word or byte) of this launch
  int64_t items = 0;     // groups (fill / copy: words or bytes) of this launch
  int64_t aux = -1;      // encode_v16, encode_gather_var, encode_scatter: first parity row; decodes, recover_gather(_var), recover_scatter: first rebuilt row of the pass;
                         // encode_bits: W; recover_runs: run-image bytes; fill / copy: bytes per
                         // work item
};
static_assert(sizeof(LaunchRecord) == 16 * sizeof(int64_t), "the reader copies 16 words per launch");
constexpr uint64_t kLaunchTraceCapacity = 1u << 16;  // records kept; later launches are only counted

void trace_launch(const LaunchRecord& rec);

// The kernels of the wide calls on a context in FEC_WIDE_ROWS_ALL for a shape with min(k, r) > 32,
// numbered on in a list of their own; named by quicfec.WIDE_DEEP_LAUNCH_FORMS.  The record builder
// is fec_wide_deep.hip's; the consumers are decode_wide and recover_scatter_wide instantiated over
// the deep record (fec_forms.hpp kDeepRecord in pol).  The classifies are kClassifyWide's and
// kClassifyTableWide's, the slots passes kDecodeWide's.
enum class WideDeepLaunchForm : int64_t {
  kBuildRecordsDeep = 33,        // first_item / items: the plan chunk's first group and its groups, one launch
                                 // per chunk, a workgroup per group; aux: 0, the arena slot of the first
  kDecodeWideDeep = 34,          // as kDecodeWide, in place
  kRecoverScatterWideDeep = 35,  // as kRecoverScatterWide
};

// The kernels of the packed recovers for every shape (fec_packed.hip: fec_recover_packed_rs_dev,
// fec_recover_packed_wide_rs_dev), numbered on in a list of their own; named by
// quicfec.PACKED_LAUNCH_FORMS.  The one-word prefix is kRowsBlockSums .. kRowsWrite's, the scan of the
// block sums kRowsScanBlocks for either mask width, the classifies and record builds their families'.
enum class PackedLaunchForm : int64_t {
  kRowsBlockSumsWide = 36,   // first_item / items: 0 and the call's groups
  kRowsWriteWide = 37,       // as kRowsWrite; direct: writes the total itself
  kRecoverPacked = 38,       // first_item / items: groups of the call; k = 0, r = 8; pol; aux: first row of the pass
  kRecoverPackedWide = 39,   // as kRecoverPacked, over a wide or a deep record
};

}  // namespace qfec
