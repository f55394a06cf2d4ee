// fec_forms.hpp — which kernel form a call runs: the launch descriptions, the lists of compiled
// shapes and the rules that choose among them.  Host-only (no HIP include, no device code), so a
// plain C++ program can ask for every packet size (tests/csrc/forms_dump.cpp; for the address-table
// calls tests/csrc/table_forms_dump.cpp).  The launchers of the kernel translation units
// (fec_encode.hip, fec_decode.hip, fec_decode_fused.hip, fec_runs.hip; the address-table units)
// dispatch on what is decided here and expand the same lists.
#pragma once

#include <cstdint>

#include "fec_knobs.hpp"

namespace qfec {

// Byte offsets of packets, when the data shards are not contiguous.
// kAddr: `offsets` holds one absolute device address per packet (u64), `data` is unused --
// the legacy-call coalescer (fec_coalesce.cpp) gathers packets from many callers' buffers.
enum class OffsetKind : int { kNone = 0, kU32 = 1, kU64 = 2, kAddr = 3 };

// Packets of any size P >= 16 at any byte address run on the 16-byte-column kernels
// (fec_encode.hip header); shorter ones on the byte kernels.
struct EncodeLaunch {
  const uint8_t* data;       // base of the data shards (device address)
  const void* offsets;       // device u32/u64 offsets (k per group) or nullptr
  OffsetKind off_kind;
  uint8_t* parity;           // parity row (g, i) at (g * r + i) * P
  uint64_t groups;
  uint32_t k, r, P;
  const void* tables;        // (r-1) x k CoefEntry (rows 1..r-1), device
  int waves_per_cu = 0;      // occupancy cap of the streaming kernel (0 = tuned default)
};

struct LevelMeta {           // codebook levels e = 1..32 (see gf256.hpp)
  uint64_t base[33];
  uint64_t stride[33];
  uint64_t count_r[33];      // C(r, e)
};

// Decode kernel selection (tests / probes; the library uses kDecodeAuto).
constexpr int kDecodeAuto = 0;           // the measured best of the forms below
constexpr int kDecodeWavePerGroup = 1;   // one wave per group, 16-B lanes only
constexpr int kDecodeTiledPlain = 2;     // workgroup = whole groups, per-lane records
constexpr int kDecodeTiledNt = 3;        //   same, non-temporal stores
constexpr int kDecodeWavePlain = 4;      // one wave per group, 16-B passes + 4-B tail
constexpr int kDecodeWaveNt = 5;         //   same, non-temporal stores (the default)
constexpr int kDecodeWaveNoBranch = 6;   //   same, no branch on coefficient 0 / 1
constexpr int kDecodeFused = 7;          // one wave per group, 16-B and 4-B pieces fused
constexpr int kDecodeFusedDirect = 8;    //   same, survivor addresses from the erasure mask

// Records built on the device, per call, for a shape whose codebook of every pattern is past its
// cap (FEC_PLAN_DEVICE; fec_plan.hip build_records): part of a decode's or a table recover's
// launch description.  arena == nullptr: the records come from the codebook.  The sizes are
// plan_arena()'s, below.
struct PlanLaunch {
  uint8_t* arena = nullptr;         // per_chunk slots of `stride` bytes, in the caller stream's workspace
  uint64_t stride = 0;              // bytes per slot, a multiple of 32
  uint64_t per_chunk = 0;           // groups whose records the arena holds at a time
  const uint8_t* matrix = nullptr;  // the r x k parity matrix, device
};

struct DecodeLaunch {
  int variant = kDecodeAuto;
  // Where rebuilt shards are stored, same layout as `data`; nullptr = in place in `data`.
  // May be a device-visible pointer to page-locked host memory (zero-copy writes).
  uint8_t* out = nullptr;
  uint8_t* data;
  const uint8_t* parity;
  const uint64_t* masks;
  uint32_t* rec_off;         // workspace, one u32 per group
  uint8_t* status;           // nullable
  const uint8_t* codebook;   // device
  const uint64_t* binom;     // device, 65 x 65
  LevelMeta meta;
  uint64_t groups;
  uint32_t k, r, P;
  int waves_per_cu = 0;      // occupancy cap of the decode kernel (0 = tuned default)
  bool rec_ready = false;    // rec_off already filled by the host (sparse plan): no classify
  int xcd_swizzle = -1;      // XCD-aware group order: -1 tuned default, 0 off, 1 on
  // Groups per wave of the mask-addressed decode (kDecodeScanGroups or 1).  One wave per
  // group is best when most groups lost data (C3: 5.35 TB/s vs 4.92 at 8 per wave); when few
  // did (C5, iid 1% loss: ~10% of groups) 8 per wave saves the dispatch and mask-load latency
  // of the waves that find nothing to do (0.257 -> 0.243 ms per 1M groups,
  // profiles/r02_probe_decode_scan.txt).  The host paths that know the masks pick it.
  uint32_t scan = 1;
  // `codebook` holds coefficient bytes (compact layout, gf256.hpp) rather than CoefEntry
  // tables: set exactly when decode_form(*this).compact_tables (launch_decode checks).
  bool compact_tables = false;
  // Rebuilt shards go to out + (g * r + m) * P (m-th lost data shard of group g, ascending),
  // `data` is only read (fec_recover_batch_rs_dev); else in place / at `out` like `data`.
  bool compact_out = false;
  // compact_out with rec_off = the packed rows' row_start (fec_recover_batch_rs_dev_packed):
  // rows are placed by global row index, so chunked launches must not offset `out`.
  bool packed_rows = false;
  // Records built on the device (plan.arena set; needs rec_ready, masks and rec_off): classify,
  // then chunk after chunk build_records and the form's passes, `codebook` being the arena.
  PlanLaunch plan;
};

constexpr uint32_t kDecodeScanGroups = 8;
// Share of groups needing a rebuild below which the host paths use the scan form.
constexpr double kDecodeScanMaxShare = 0.25;

// Packed recover in one launch (recover_runs, fec_runs.hip): every workgroup owns 512
// consecutive groups, finds its run's first row by decoupled look-back (no prefix launches)
// and writes its rebuilt rows as one contiguous run, staged through an LDS image of up to
// stage bytes.  Mask-addressed shapes only (runs_supported).
struct RunsLaunch {
  const uint8_t* data;
  const uint8_t* parity;
  const uint64_t* masks;
  uint64_t groups;
  uint32_t k, r, P;
  const uint8_t* codebook;   // dense CoefEntry codebook (the mask-addressed decode's)
  LevelMeta meta;
  uint8_t* out;              // packed rows
  uint32_t* row_start;       // one u32 per group (written)
  uint64_t* total;           // nullable: all rows
  uint8_t* status;           // nullable
  // runs_workspace_bytes(groups) of device memory, zeroed when first allocated, kept by the
  // caller stream: ticket counter, chunk totals, look-back words
  void* workspace;
  // look-back epoch of the first launch; a call takes runs_launches(groups) epochs, never
  // reused while the workspace lives (the caller counts; < 2^30, then re-zero the workspace)
  uint32_t epoch;
  int stage_bytes = -1;      // LDS run image: -1 tuned default (test switch kRunsStage), 0 none
};

// The look-back epochs of a call of n launches on a workspace whose last launch used epoch
// `last` (0: none since the workspace was zeroed): first .. first + n - 1, each non-zero and
// below `limit`, none handed out twice while the workspace's words live.  When they would reach
// the limit the workspace must be zeroed first (`rezero`) and the count starts again at 1.
// Needs n < limit.  The epoch is the 30 bits above bit 34 of a look-back word (fec_runs.hip
// kRunEpochShift), so the limit is 2^30 (the test library's TestKnob::kRunsEpochLimit lowers it).
constexpr uint32_t kRunsEpochLimit = 1u << 30;
struct RunsEpochs {
  uint32_t first;
  bool rezero;
};
constexpr RunsEpochs runs_epochs(uint32_t last, uint32_t n, uint32_t limit) {
  const bool rezero = static_cast<uint64_t>(last) + n >= limit;
  return {(rezero ? 0u : last) + 1u, rezero};
}

// Memory policy bits of the streaming kernels.
constexpr int kNtLoad = 1;        // non-temporal loads (data read once)
constexpr int kNtStore = 2;       // non-temporal stores
constexpr int kNoCoefBranch = 4;  // decode: multiply by every coefficient, no 0/1 branches
// decode_fused: coefficient tables through LDS.  A record-addressed wave reads e*K 32-B
// table entries of its group's record.  For large codebooks (k=20 r=5: 53,130 records,
// 143 MB) the records miss the scalar cache, and one scalar load per coefficient — a few
// in flight at a time — stalls the wave for several memory round trips per group.  With
// this bit the wave fetches its rows with vector loads issued next to its survivor loads
// (one round trip) and reads them from a per-wave LDS slice.
constexpr int kLdsTabs = 64;
// decode_fused / decode_wave: the m-th rebuilt shard of group g (erased data shards in
// ascending order) goes to out + (g * r + m) * P -- one contiguous run of rebuilt packets
// per group, groups back to back, like encode's parity rows -- instead of its place among
// the group's data shards (fec_recover_batch_rs_dev).  Measured at k=10 r=3, 2 erasures:
// 2.32 vs 2.47 ms in place (profiles/r02_probe_decode_compact_out.txt).
constexpr int kCompactOut = 1024;
// decode_fused with kLdsTabs: the record holds bare coefficient bytes (compact codebook,
// gf256.hpp) and the wave computes each coefficient's tables into its LDS slice
// (coef_tables.hpp) instead of copying 32-byte table entries in: k=20 r=5 records shrink
// from up to 3.3 KB to 256 B, the whole codebook from 143 MB to 12 MB.
constexpr int kCoefBytes = 2048;
// encode_v16: coefficients taken two at a time, so every 3-input XOR (v_bitop3) folds two
// new table products into the accumulator: 6 v_perm + 3 v_bitop3 per pair of coefficients
// and dword instead of 6 v_perm + 2 v_bitop3 + 2 v_xor, and one v_bitop3 per pair on the
// XOR row instead of two v_xor.
constexpr int kPairMac = 4096;
// encode_v16 / encode_bits (tiled, P % 16 == 0, every row of the code in this launch): the
// workgroup's parity rows -- one contiguous window of tile * R * P bytes in HBM -- are staged in
// the LDS the launch already reserves for its occupancy cap and stored by consecutive lanes as
// consecutive 16-B pieces, so only the window's two end lines are partial.  Stored by the lanes
// that computed them, a 1200-B row starts 48 B into a 128-B line and one store instruction
// covers the end of one group's row and the start of another's: each row's edge lines leave as
// pieces of different instructions (PMC writes 1.046x algorithmic at k=10 r=3, 1.053x at k=20
// r=5).
constexpr int kStageRows = 8192;
constexpr int kEncodeStageDefault = 1;  // on: C2 encode 2.753 -> 2.659 ms, C4 5.578 -> 5.520 (profiles/r05a)

constexpr uint32_t kVecMinP = 16;  // shorter packets take the byte kernels
// Packets of at most this size decode in the tiled form (several groups per wave).
constexpr uint32_t kTiledMaxP = 256;

// ---- the compiled shapes, each list stated once ----
// A list macro calls M(extra..., k, r) per shape (M(extra..., nm, nt) per layout); the predicates
// below, the launchers' dispatch and the test program's --compiled list are expansions of these.
// Mask-addressed decode_fused and recover_runs.  r <= 3 shapes only in the mask-addressed form
// (the one auto uses for them), r > 3 only in the record-addressed one; k=10 r=3 1200 B in both
// (probes).
#define QFEC_MASK_SHAPES(M, ...) M(__VA_ARGS__, 10, 3) M(__VA_ARGS__, 10, 1) M(__VA_ARGS__, 10, 2) M(__VA_ARGS__, 4, 2)
// k=10 r=3 (the BASELINE shape) also has the scan form, for sparse loss (DecodeLaunch::scan)
#define QFEC_SCAN_SHAPES(M, ...) M(__VA_ARGS__, 10, 3)
// The r > 3 record-addressed forms stage their tables
// through LDS (kLdsTabs): k=20 r=5, 5 erasures, 1200 B: 2.27 -> 4.73-4.92 TB/s
// (profiles/r01_probe_decode_ldstabs_k20.txt); at k=10 r=3, whose 286 records stay in the
// scalar cache, it gains nothing (profiles/r01_probe_decode_inline_k10.txt).
#define QFEC_LDS_SHAPES(M, ...) M(__VA_ARGS__, 20, 5)
// Record-addressed with CoefEntry records (host-built records, probes): one shape at one layout.
#define QFEC_RECORD_FORMS(M, ...) M(__VA_ARGS__, 10, 3, 1, 1)
#define QFEC_TILED_SHAPES(M, ...) M(__VA_ARGS__, 10, 3) M(__VA_ARGS__, 10, 1) M(__VA_ARGS__, 20, 5) M(__VA_ARGS__, 4, 2)
// compile-time-k decode_wave (and the probes' decode_v16)
#define QFEC_WAVE_SHAPES(M, ...) QFEC_TILED_SHAPES(M, __VA_ARGS__)
// probes only: decode_wave without the branch on coefficients 0 / 1
#define QFEC_WAVE_NB_SHAPES(M, ...) M(__VA_ARGS__, 10, 3) M(__VA_ARGS__, 20, 5)
// The piece layouts of decode_fused and recover_runs.
// Instantiated for every P in [16, 2047] of the compiled (k, r) shapes: NM = P / 1024 16-B and
// NT = ceil((P % 1024) / 256) 4-B pieces per lane, (NM, NT) in (0,1..4), (1,0..4); P = 2048 would
// be (2,0), which is not instantiated, so 2048 and up take the wave kernel.  P <= 256 is the one
// 4-B piece (0,1): the shapes with a tiled form decode such packets there in both layouts, so of
// the mask-addressed (0,1) forms only k=10 r=2's compact one is ever launched (recover layouts);
// k=10 r=2 in place at P <= 256 goes to the runtime-k wave kernel (a known slow
// path).
// Measured at k=10 r=3, 2 erasures (tools/probe_decode.hip): 512 B 5.89 TB/s vs 3.12 for
// the looped wave kernel, 768 B 5.49 vs 3.24 (profiles/r01_probe_decode_small.txt).
#define QFEC_LAYOUTS(M, ...)                                                                      \
  M(__VA_ARGS__, 0, 1) M(__VA_ARGS__, 0, 2) M(__VA_ARGS__, 0, 3) M(__VA_ARGS__, 0, 4) M(__VA_ARGS__, 1, 0) \
  M(__VA_ARGS__, 1, 1) M(__VA_ARGS__, 1, 2) M(__VA_ARGS__, 1, 3) M(__VA_ARGS__, 1, 4)

#define QFEC_IS_PAIR(_, A, B) || (a == A && b == B)
constexpr bool is_mask_shape(uint32_t a, uint32_t b) { return false QFEC_MASK_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_scan_shape(uint32_t a, uint32_t b) { return false QFEC_SCAN_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_lds_shape(uint32_t a, uint32_t b) { return false QFEC_LDS_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_tiled_shape(uint32_t a, uint32_t b) { return false QFEC_TILED_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_wave_shape(uint32_t a, uint32_t b) { return false QFEC_WAVE_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_wave_nb_shape(uint32_t a, uint32_t b) { return false QFEC_WAVE_NB_SHAPES(QFEC_IS_PAIR, ~); }
constexpr bool is_layout(uint32_t a, uint32_t b) { return false QFEC_LAYOUTS(QFEC_IS_PAIR, ~); }
#undef QFEC_IS_PAIR
#define QFEC_IS_QUAD(_, K, R, A, B) || (k == K && r == R && nm == A && nt == B)
constexpr bool is_record_form(uint32_t k, uint32_t r, uint32_t nm, uint32_t nt) {
  return false QFEC_RECORD_FORMS(QFEC_IS_QUAD, ~);
}
#undef QFEC_IS_QUAD

struct Layout {
  uint32_t nm, nt;  // 16-B and 4-B pieces per lane
};
constexpr Layout layout_of(uint32_t P) { return {P / 1024u, (P % 1024u + 255u) / 256u}; }
constexpr bool has_layout(uint32_t P) { return P >= kVecMinP && is_layout(layout_of(P).nm, layout_of(P).nt); }
static_assert(has_layout(16) && has_layout(2047) && !has_layout(15) && !has_layout(2048) && !has_layout(4096),
              "a layout exists for 16 <= P <= 2047");

// The kernel instantiations of the product library's decode dispatch, X(kernel, K, MAXE, NM, NT,
// POL, DIRECT, SCAN); QFEC_PROBE_DECODE_FORMS: those only the probes select (compiled with
// QUICFEC_PROBE_FORMS); QFEC_RUNS_FORMS: recover_runs, X(K, R, NM, NT).
// The mask-addressed forms also load non-temporally (survivors are read once): +1.2..3.2% at
// 512 / 768 / 1200 / 1400 B in one process (profiles/r01_probe_decode_ntload.txt); loads
// alone without NT stores lose 14%.
#define QFEC_FORM_MASK(X, K, R, NM, NT)                        \
  X(kFused, K, R, NM, NT, kNtStore | kNtLoad, true, 0) X(kFused, K, R, NM, NT, kNtStore | kNtLoad | kCompactOut, true, 0)
#define QFEC_FORM_SCAN(X, K, R, NM, NT)                                \
  X(kFused, K, R, NM, NT, kNtStore | kNtLoad, true, kDecodeScanGroups) \
  X(kFused, K, R, NM, NT, kNtStore | kNtLoad | kCompactOut, true, kDecodeScanGroups)
#define QFEC_FORM_LDS(X, K, R, NM, NT)                                           \
  X(kFused, K, R, NM, NT, kNtStore | kNtLoad | kLdsTabs | kCoefBytes, false, 0) \
  X(kFused, K, R, NM, NT, kNtStore | kNtLoad | kLdsTabs | kCoefBytes | kCompactOut, false, 0)
#define QFEC_FORM_RECORD(X, K, R, NM, NT) X(kFused, K, R, NM, NT, kNtStore, false, 0)
#define QFEC_FORM_TILED(X, K, R) X(kTiled, K, R, 0, 0, kNtStore, false, 0) X(kTiled, K, R, 0, 0, kNtStore | kCompactOut, false, 0)
#define QFEC_FORM_WAVE(X, K, R) X(kWave, K, R, 0, 0, kNtStore, false, 0)
#define QFEC_FORM_RUNS(X, K, R, NM, NT) X(K, R, NM, NT)
#define QFEC_MASK_LAYOUTS(X, K, R) QFEC_LAYOUTS(QFEC_FORM_MASK, X, K, R)
#define QFEC_SCAN_LAYOUTS(X, K, R) QFEC_LAYOUTS(QFEC_FORM_SCAN, X, K, R)
#define QFEC_LDS_LAYOUTS(X, K, R) QFEC_LAYOUTS(QFEC_FORM_LDS, X, K, R)
#define QFEC_RUNS_LAYOUTS(X, K, R) QFEC_LAYOUTS(QFEC_FORM_RUNS, X, K, R)
// Two lists, one per translation unit: decode_fused's forms (fec_decode_fused.hip) and the others
// (fec_decode.hip); each unit expands its own, QFEC_DECODE_FORMS is both.
#define QFEC_DECODE_FUSED_FORMS(X)                                                                \
  QFEC_MASK_SHAPES(QFEC_MASK_LAYOUTS, X) QFEC_SCAN_SHAPES(QFEC_SCAN_LAYOUTS, X)                   \
  QFEC_LDS_SHAPES(QFEC_LDS_LAYOUTS, X) QFEC_RECORD_FORMS(QFEC_FORM_RECORD, X)
#define QFEC_DECODE_OTHER_FORMS(X)                                                                \
  QFEC_TILED_SHAPES(QFEC_FORM_TILED, X) QFEC_WAVE_SHAPES(QFEC_FORM_WAVE, X)                       \
  X(kWave, 0, 8, 0, 0, kNtStore | kNoCoefBranch, false, 0)                                        \
  X(kWave, 0, 8, 0, 0, kNtStore | kNoCoefBranch | kCompactOut, false, 0)                          \
  X(kBytes, 0, 0, 0, 0, 0, false, 0) X(kBytes, 0, 0, 0, 0, kCompactOut, false, 0)
#define QFEC_DECODE_FORMS(X) QFEC_DECODE_FUSED_FORMS(X) QFEC_DECODE_OTHER_FORMS(X)
#define QFEC_RUNS_FORMS(X) QFEC_MASK_SHAPES(QFEC_RUNS_LAYOUTS, X)
#define QFEC_FORM_TILED_PLAIN(X, K, R) X(kTiled, K, R, 0, 0, 0, false, 0)
#define QFEC_FORM_WAVE_PLAIN(X, K, R) X(kWave, K, R, 0, 0, 0, false, 0) X(kV16, K, R, 0, 0, 0, false, 0)
#define QFEC_FORM_WAVE_NB(X, K, R) X(kWave, K, R, 0, 0, kNtStore | kNoCoefBranch, false, 0)
// (no decode_fused form among them: the probes launch theirs by hand, so the list is fec_decode.hip's)
#define QFEC_PROBE_DECODE_FORMS(X)                                                                \
  QFEC_TILED_SHAPES(QFEC_FORM_TILED_PLAIN, X) QFEC_WAVE_SHAPES(QFEC_FORM_WAVE_PLAIN, X)           \
  QFEC_WAVE_NB_SHAPES(QFEC_FORM_WAVE_NB, X) X(kWave, 0, 8, 0, 0, 0, false, 0) X(kV16, 0, 8, 0, 0, 0, false, 0)
// The compile-time encodes, X(K, R, OFF, POL) (the runtime-k passes and the byte kernel are the
// launcher's): encode_v16 and encode_bits (W = 4).
#define QFEC_ENCODE_V16_FORMS(X)                                                                  \
  X(10, 3, 0, kNtStore | kPairMac) X(10, 3, 0, kNtStore | kPairMac | kStageRows) X(10, 2, 0, kNtStore | kPairMac) \
  X(10, 2, 0, kNtStore | kPairMac | kStageRows) X(20, 5, 0, kNtStore | kPairMac) X(10, 1, 0, kNtStore)            \
  X(4, 2, 0, kNtStore) X(10, 1, 1, kNtStore) X(10, 1, 3, kNtStore)
#define QFEC_ENCODE_BITS_FORMS(X) \
  X(20, 5, 0, kNtStore) X(20, 5, 0, kNtStore | kStageRows) X(10, 3, 0, kNtStore) X(10, 3, 0, kNtStore | kStageRows)

// Groups per workgroup for the tiled mapping: the fewest idle lanes (workgroup = whole
// waves), preferring tiles whose byte size is a multiple of 128 (tile starts stay
// cache-line aligned).  0 = use the flat mapping (columns per packet > 512).
inline uint32_t pick_tile(uint32_t cpp, uint32_t k, uint32_t P) {
  if (cpp == 0 || cpp > 512) return 0;
  const uint32_t tmax = 512 / cpp;
  uint32_t best = 1;
  double best_score = 1e9;
  for (uint32_t t = 1; t <= tmax; ++t) {
    const uint32_t lanes = t * cpp, bs = (lanes + 63) / 64 * 64;
    double score = double(bs - lanes) / bs;
    if ((uint64_t(t) * k * P) % 128 != 0) score += 0.05;
    if (bs < 256) score += 0.02;
    if (score < best_score - 1e-9) {
      best_score = score;
      best = t;
    }
  }
  return best;
}

// ---- decode ----
enum class DecodeKernel : int { kNone = 0, kBytes, kTiled, kFused, kWave, kV16 };

// Everything launch_decode and its caller need to know about one call.
struct DecodeForm {
  DecodeKernel kernel = DecodeKernel::kNone;  // kNone: no groups, nothing to launch
  int K = 0, MAXE = 0;          // template shape; runtime k as K = 0, MAXE = 8
  int NM = 0, NT = 0;           // decode_fused: piece layout
  int POL = 0;
  bool DIRECT = false;          // decode_fused: mask-addressed, classifies inline
  int SCAN = 0;                 // decode_fused: groups per wave of the scan form, 0 = one wave per group
  uint32_t tile = 0;            // decode_tiled: groups per workgroup
  bool classify = false;        // a classify launch precedes the kernel
  bool rec_off = false;         // reads the rec_off workspace (every form but the mask-addressed
                                // one): the caller then provides a workspace private to the call
  bool compact_tables = false;  // reads a compact codebook (coefficient bytes)
};

// The form launch_decode(a) runs.  A form that is compiled only with QUICFEC_PROBE_FORMS (a
// probe's variant; the library never sets one) is named here too: the product library's
// dispatch answers it with hipErrorNotSupported.
inline DecodeForm decode_form(const DecodeLaunch& a) {
  using DK = DecodeKernel;
  DecodeForm f;
  if (a.groups == 0) return f;
  const int compact = a.compact_out ? kCompactOut : 0;
  const auto pick = [&f](DK kernel, uint32_t k, uint32_t maxe, int pol) {
    f.kernel = kernel, f.K = static_cast<int>(k), f.MAXE = static_cast<int>(maxe), f.POL = pol;
    return f;
  };
  f.classify = !a.rec_ready;
  f.rec_off = true;
  if (a.P < kVecMinP) return pick(DK::kBytes, 0, 0, compact);
  const Layout lay = layout_of(a.P);
  f.tile = pick_tile((a.P + 15u) / 16u, a.k, a.P);
  // The tiled route: the compact recover layout only where a tiled form is compiled; elsewhere
  // the fused or wave forms write it.  In place, a shape without a tiled form still takes this
  // route and falls through to its wave kernel below (k=10 r=2 at P <= 256, the known slow path).
  // auto leaves k=20 r=5 to the LDS-table fused form (P=200: 4.6 vs 2.8 TB/s, same box)
  const bool auto_tiled = a.variant == kDecodeAuto && a.P <= kTiledMaxP && !is_lds_shape(a.k, a.r);
  const bool tiled = !(a.compact_out && !is_tiled_shape(a.k, a.r)) && f.tile > 0 &&
                     (auto_tiled || a.variant == kDecodeTiledPlain || a.variant == kDecodeTiledNt);
  // Mask-addressed fused form (r <= 3): +1.2% at k=10 r=3 (tools/probe_decode.hip,
  // r01_probe_decode_direct.txt); at k=20 r=5 its extra VGPRs cost a wave per SIMD (-30%), so
  // auto takes it for r <= 3 only.  It classifies inline: one launch, no classify kernel.
  if (!tiled && a.masks != nullptr && !a.rec_ready &&
      (a.variant == kDecodeFusedDirect || (a.variant == kDecodeAuto && a.r <= 3)) && is_mask_shape(a.k, a.r) &&
      has_layout(a.P)) {
    f.classify = f.rec_off = false;
    f.NM = static_cast<int>(lay.nm), f.NT = static_cast<int>(lay.nt), f.DIRECT = true;
    f.SCAN = is_scan_shape(a.k, a.r) && a.scan == kDecodeScanGroups ? static_cast<int>(kDecodeScanGroups) : 0;
    return pick(DK::kFused, a.k, a.r, kNtStore | kNtLoad | compact);
  }
  // packets <= 256 B: the tiled form (several groups per wave); plain stores are probe-only
  if (tiled && is_tiled_shape(a.k, a.r))
    return pick(DK::kTiled, a.k, a.r, (a.compact_out || a.variant != kDecodeTiledPlain ? kNtStore : 0) | compact);
  // Fused passes win where many rows share each survivor (k=20 r=5, 5 losses: +21%); with
  // the XCD-aware order they also win at r = 3 (+2.6%; tools/probe_decode.hip), so auto
  // takes them wherever they are instantiated.
  if ((a.variant == kDecodeFused || a.variant == kDecodeAuto || a.variant == kDecodeFusedDirect) && has_layout(a.P)) {
    f.NM = static_cast<int>(lay.nm), f.NT = static_cast<int>(lay.nt);
    if (!a.compact_out && is_record_form(a.k, a.r, lay.nm, lay.nt)) return pick(DK::kFused, a.k, a.r, kNtStore);
    if (is_lds_shape(a.k, a.r)) {
      f.compact_tables = !a.rec_ready;  // host-built records are CoefEntry tables
      return pick(DK::kFused, a.k, a.r, kNtStore | kNtLoad | kLdsTabs | kCoefBytes | compact);
    }
    f.NM = f.NT = 0;
  }
  // everything else: the wave kernel; compact only at runtime k
  if (a.compact_out) return pick(DK::kWave, 0, 8, kNtStore | kNoCoefBranch | kCompactOut);
  // Probe-only forms (tools/probe_decode.hip sets DecodeLaunch::variant; the library never does):
  // no branch on coefficients 0 / 1, the plain-store wave kernel, 16-B lanes only (decode_v16).
  const bool separate_out = a.out != nullptr && a.out != a.data;  // decode_v16 lacks it
  if (a.variant == kDecodeWaveNoBranch && !separate_out && is_wave_nb_shape(a.k, a.r))
    return pick(DK::kWave, a.k, a.r, kNtStore | kNoCoefBranch);
  if (a.variant == kDecodeWavePerGroup && !separate_out)
    return is_wave_shape(a.k, a.r) ? pick(DK::kV16, a.k, a.r, 0) : pick(DK::kV16, 0, 8, 0);
  const bool nt = a.variant != kDecodeWavePlain;
  if (is_wave_shape(a.k, a.r)) return pick(DK::kWave, a.k, a.r, nt ? kNtStore : 0);
  // Runtime k: multiplying by every coefficient (no branches on 0 / 1) wins at every shape
  // measured (tools/probe_decode.hip, profiles/r01_probe_decode_runtime_k.txt): k=10 r=2
  // 4.13 -> 4.79 TB/s, 12+6 2.62 -> 3.20, 16+4 2.67 -> 3.40.  Its tables staged through
  // LDS (kLdsTabs) lose here (2.2-2.8 TB/s): the records of these codebooks are hit often
  // enough in the scalar cache, and the wait for the tables precedes the survivor loads.
  return pick(DK::kWave, 0, 8, nt ? kNtStore | kNoCoefBranch : 0);
}

// (k, r, P) shapes with a compiled recover_runs: the mask-addressed decode's, 256 < P <= 2047
// or 16 <= P <= 256 with one 4-B piece (the packed call reaches the latter only for k=10 r=2:
// the other shapes' short packets are refused, their slot layout being the tiled form's).
constexpr bool runs_supported(uint32_t k, uint32_t r, uint32_t P) { return is_mask_shape(k, r) && has_layout(P); }

// What fec_recover_batch_rs_dev_packed does with call `a` (compact_out and the scan setting
// set, rec_off and packed_rows not yet) of form f = decode_form(a); `runs_switch` is the test
// library's TestKnob::kPackedRuns (-1 unset).
enum class PackedForm : int { kRefused, kRuns, kPrefixFused };
inline PackedForm packed_form(const DecodeLaunch& a, const DecodeForm& f, long runs_switch) {
  // packed rows: only the mask-addressed (inline-classify) forms place rows by row_start,
  // which they read from rec_off
  if (a.rec_ready || f.rec_off) return PackedForm::kRefused;
  // Sparse loss (the scan form's share): one launch, recover_runs --
  // each workgroup finds its rows' place by decoupled look-back and writes them as one run
  // (C5: 0.229-0.235 vs 0.242-0.268 ms for the slot rows; profiles/r04_probe_runs_*.txt).
  // Dense loss keeps the prefix launches + decode_fused (the runs form rebuilds a workgroup's
  // groups wave by wave: 2.7-2.8 vs 2.2-2.45 ms at C3).  The test library's
  // TestKnob::kPackedRuns forces it on (1) or off (0).
  if (runs_switch != 0 && (runs_switch == 1 || a.scan == kDecodeScanGroups) && runs_supported(a.k, a.r, a.P))
    return PackedForm::kRuns;
  return PackedForm::kPrefixFused;
}

// ---- the address-table calls (fec_gather.hip, fec_gather_var.hip, fec_scatter.hip,
// fec_scatter_encode.hip) ----
// Shards wherever they are in device memory: a table of absolute addresses per group (0 = lost /
// absent), optionally a u32 length per entry, indexed alike -- shard (g, s) is then the bytes
// [0, min(len, P)) at its address, zeros up to P (fec_varlen.hpp) -- and optionally a table of
// destinations instead of an output buffer, each written exactly the group's symbol length (the
// largest min(len, P) of its present entries; fec_scatter_cut.hpp, fec_scatter_encode_cut.hpp).
//
// A recover (fec_recover_gather_rs_dev, fec_recover_gather_var_rs_dev, fec_recover_scatter_rs_dev).
struct TableRecoverLaunch {
  const uint64_t* addrs;     // groups * (k + r) absolute device addresses, 0 = lost
  const uint32_t* lens;      // groups * (k + r) readable bytes per entry, a lost entry's ignored: the
                             // variable-length gather's; the scatter's, nullable (NULL = every present
                             // shard has P); not read by the fixed-length gather
  const uint64_t* dests;     // the scatter's: groups * k absolute device addresses, 0 = not wanted
  uint64_t groups;
  uint32_t k, r, P;
  uint8_t* out;              // the gathers': rebuilt row (g, m) at (g * r + m) * P; not used by the scatter
  uint8_t* status;           // nullable
  uint64_t* masks_out;       // nullable: the erasure mask derived for each group
  uint32_t* symlen;          // per group its symbol length, 0 when no entry is present.  The
                             // variable-length gather's nullable output; the scatter's output or, when
                             // the caller gives none and there is a length table, workspace (its kernel
                             // reads it); not used by the fixed-length gather
  uint32_t* rec_off;         // workspace, one u32 per group
  const uint8_t* codebook;   // dense CoefEntry codebook (the one `classify` addresses), device
  const uint64_t* binom;     // device, 65 x 65
  LevelMeta meta;
  bool rec_ready = false;    // rec_off already holds the records of `codebook` (a chunk of a device
                             // plan): no classify, as DecodeLaunch::rec_ready
  PlanLaunch plan;           // records built on the device (plan.arena set; needs masks_out): classify,
                             // then chunk after chunk build_records and the call's passes
};

// An encode (fec_encode_gather_var_rs_dev, fec_encode_scatter_rs_dev).  Exactly one of `parity`
// (the gather's) and `dests` (the scatter's) is set.
struct TableEncodeLaunch {
  const uint64_t* addrs;     // groups * k absolute device addresses, 0 = absent (counts as zeros)
  const uint32_t* lens;      // groups * k readable bytes per packet: the gather's; the scatter's,
                             // nullable (NULL = every present packet has P)
  uint64_t groups;
  uint32_t k, r, P;
  uint8_t* parity;           // parity row (g, i) at (g * r + i) * P, full P-byte rows
  const uint64_t* dests;     // groups * r absolute device addresses, 0 = not wanted
  uint32_t* symlen_out;      // nullable
  const void* tables;        // (r-1) x k CoefEntry (rows 1..r-1), device
};

// The compiled shapes of the table recovers, M(extra, k, r), and the instantiations of each of
// their kernels (recover_gather, recover_gather_var, recover_scatter), X(extra, K, MAXE, POL) with
// one extra argument (`~` for none): a list of their own, apart from the decode lists above.  Every
// form loads and stores non-temporally and has the compact slot layout in POL, like the slot
// recover's mask-addressed form (the scatter's rows go to the destination table whatever it says);
// runtime k takes passes of 8 rows and multiplies by every coefficient (as the runtime-k
// decode_wave does).
#define QFEC_GATHER_SHAPES(M, ...) \
  M(__VA_ARGS__, 10, 3) M(__VA_ARGS__, 10, 2) M(__VA_ARGS__, 10, 1) M(__VA_ARGS__, 4, 2) M(__VA_ARGS__, 20, 5)
constexpr int kGatherPol = kNtStore | kNtLoad | kCompactOut;
#define QFEC_TABLE_RECOVER_FIXED(X, A, K, R) X(A, K, R, kGatherPol)
#define QFEC_TABLE_RECOVER_FORMS(X, ...) \
  QFEC_GATHER_SHAPES(QFEC_TABLE_RECOVER_FIXED, X, __VA_ARGS__) X(__VA_ARGS__, 0, 8, kGatherPol | kNoCoefBranch)
#define QFEC_IS_PAIR(_, A, B) || (a == A && b == B)
constexpr bool is_gather_shape(uint32_t a, uint32_t b) { return false QFEC_GATHER_SHAPES(QFEC_IS_PAIR, ~); }
#undef QFEC_IS_PAIR

struct TableRecoverForm {
  bool supported = false;  // false: P < 16, the call is refused
  int K = 0, MAXE = 0;     // template shape; runtime k as K = 0, MAXE = 8
  int POL = 0;
  bool VAR = false;        // with a length table: loads masked by it (the scatter: stores cut at the symbol length)
};

// The form a table recover runs for (k, r, P) with (var) or without a length table: a classify
// launch, then the call's kernel <K, MAXE, POL> (the scatter's: <K, MAXE, POL, VAR>) in
// ceil(r / MAXE) passes.  The kernels walk the pieces of any P >= 16 themselves, so the size only
// decides whether the call is served, and the length table never chooses a shape.  Every form
// takes its records from the dense CoefEntry codebook; k=20 r=5 too (no compact-codebook /
// LDS-table form).
inline TableRecoverForm table_recover_form(uint32_t k, uint32_t r, uint32_t P, bool var) {
  TableRecoverForm f;
  if (P < kVecMinP) return f;
  f.supported = true, f.VAR = var;
  if (is_gather_shape(k, r)) {
    f.K = static_cast<int>(k), f.MAXE = static_cast<int>(r), f.POL = kGatherPol;
  } else {
    f.K = 0, f.MAXE = 8, f.POL = kGatherPol | kNoCoefBranch;
  }
  return f;
}

// ---- records built on the device (FEC_PLAN_DEVICE; fec_plan.hip, fec_plan_build.hpp) ----
// A shape whose codebook of every pattern is past its cap has no record to look up.  With the
// context in FEC_PLAN_DEVICE each group's record is built on the device into an arena of slots in
// the caller stream's workspace, right before the kernels that read it; those are the runtime-k
// record-addressed forms (decode_wave<0, 8>, the table recovers' <0, 8>, decode_bytes), which read
// a record at codebook + rec_off[g] * 32 wherever it came from.
//
// A slot holds the largest record of the shape, record_bytes(k, min(k, r)) (gf256.hpp: a 128-B
// header, then 32 B per row and survivor), a multiple of 32.
constexpr uint64_t plan_slot_stride(uint32_t k, uint32_t r) { return 128u + uint64_t{k < r ? k : r} * k * 32u; }
// The arena's budget per caller stream: the size of a host-pipeline chunk (kPipeChunkBytes).  A
// cap on memory, not a tuned number: at most 16 stream workspaces exist (fec_shim.cpp), so 1 GiB
// in all.  The test library's TestKnob::kPlanArenaBytes lowers it.
constexpr uint64_t kPlanArenaBytes = 64ull << 20;
inline uint64_t plan_arena_budget() {
  const long n = test_knob(TestKnob::kPlanArenaBytes, 0);
  return n > 0 && static_cast<uint64_t>(n) < kPlanArenaBytes ? static_cast<uint64_t>(n) : kPlanArenaBytes;
}
// rec_off values a record may have: below the markers kRecBad, kRecNone (fec_kernels.hpp).
constexpr uint32_t kPlanRecLimit = 0xFFFFFFFEu;
// The arena of a call of G groups under `budget`: max(1, budget / stride) slots, at most G.  The
// call walks its groups in chunks of per_chunk: group i of a chunk has its record in slot i,
// rec_off = i * stride / 32 -- no atomics, no compaction -- and the arena is reused chunk after
// chunk in stream order.  Groups with nothing to rebuild leave their slot unwritten and unread.
struct PlanArena {
  uint64_t stride, per_chunk, bytes;  // bytes = per_chunk * stride
};
inline PlanArena plan_arena(uint32_t k, uint32_t r, uint64_t G, uint64_t budget) {
  const uint64_t stride = plan_slot_stride(k, r);
  uint64_t per = budget / stride;
  if (per == 0) per = 1;
  if (per > G) per = G;
  return {stride, per, per * stride};
}
inline uint32_t plan_slot_rec(const PlanArena& a, uint64_t slot) { return static_cast<uint32_t>(slot * (a.stride / 32u)); }
// The chunks of the walk, in order: f(first group, groups) for [0, G) in pieces of per_chunk, until
// f returns false (fec_launch.hpp for_plan_chunks launches through it).
template <typename F>
inline bool plan_chunks(uint64_t G, uint64_t per_chunk, F f) {
  for (uint64_t g0 = 0; g0 < G; g0 += per_chunk)
    if (!f(g0, G - g0 < per_chunk ? G - g0 : per_chunk)) return false;
  return true;
}
// The workspace of a device-plan call, byte offsets from its start: G record offsets; G masks (a
// table recover whose caller gives no d_masks_out: build_records reads the masks the classify
// derived); G symbol lengths (the scatter recover with a length table whose caller asks for none,
// as in codebook mode); the arena, 256-B aligned.  A region not needed is empty.
struct PlanWorkspace {
  uint64_t rec_off, masks, symlen, arena, bytes;
};
inline PlanWorkspace plan_workspace(uint64_t G, bool own_masks, bool own_symlen, const PlanArena& a) {
  PlanWorkspace w{};
  w.rec_off = 0;
  w.masks = (G * sizeof(uint32_t) + 7u) & ~uint64_t{7};
  w.symlen = w.masks + (own_masks ? G * sizeof(uint64_t) : 0);
  w.arena = (w.symlen + (own_symlen ? G * sizeof(uint32_t) : 0) + 255u) & ~uint64_t{255};
  w.bytes = w.arena + a.bytes;
  return w;
}
// Groups [g0, g0 + gn) of call `a` as a launch of their own, their records ready in the arena.
inline DecodeLaunch plan_chunk(const DecodeLaunch& a, uint64_t g0, uint64_t gn) {
  DecodeLaunch c = a;
  const uint64_t P = a.P;
  c.data = a.data + g0 * a.k * P;
  c.parity = a.parity + g0 * a.r * P;
  c.masks = a.masks + g0;
  c.rec_off = a.rec_off + g0;
  if (a.status) c.status = a.status + g0;
  if (a.out) c.out = a.out + g0 * (a.compact_out ? a.r : a.k) * P;
  c.groups = gn;
  c.rec_ready = true;
  c.codebook = a.plan.arena;
  c.plan = PlanLaunch{};
  return c;
}
inline TableRecoverLaunch plan_chunk(const TableRecoverLaunch& a, uint64_t g0, uint64_t gn) {
  TableRecoverLaunch c = a;
  const uint64_t n = a.k + a.r;
  c.addrs = a.addrs + g0 * n;
  if (a.lens) c.lens = a.lens + g0 * n;
  if (a.dests) c.dests = a.dests + g0 * a.k;
  if (a.out) c.out = a.out + g0 * a.r * static_cast<uint64_t>(a.P);
  if (a.status) c.status = a.status + g0;
  if (a.masks_out) c.masks_out = a.masks_out + g0;
  if (a.symlen) c.symlen = a.symlen + g0;
  c.rec_off = a.rec_off + g0;
  c.groups = gn;
  c.rec_ready = true;
  c.codebook = a.plan.arena;
  c.plan = PlanLaunch{};
  return c;
}

// ---- wide shapes: k + r <= 256 with four-word masks (fec_decode_wide_rs_dev, fec_recover_wide_rs_dev;
// fec_wide.hip, fec_mask_wide.hpp, fec_plan_build_wide.hpp) ----
// A wide shape is one more shape without a codebook: every call builds its records on the device,
// whatever fec_decode_plan_mode says, into an arena sized by plan_arena's arithmetic with the wide
// slot below.  The record builder inverts an e x e matrix in a per-wave LDS slice, e <= min(k, r):
// about 9.5 KiB at e = 32; e = 128 would take 48 KiB per wave, 192 KiB for a workgroup of four
// waves against the CU's 160 KiB.  Hence min(k, r) <= 32.
constexpr uint32_t kWideMaxShards = 256;
constexpr uint32_t kWideMaxRows = 32;      // min(k, r), so e
constexpr uint64_t kWideHeader = 512;      // fec_plan_build_wide.hpp kWideHeaderBytes
constexpr uint32_t kWidePassRows = 8;      // rows per pass of decode_wide (decode_piece<0, 8>)
// Whether the wide calls serve (k, r, P, G), and if not, why: the one statement of that rule.
enum class WideRefusal : int { kServed = 0, kShape, kRows, kPacket, kNoGroups, kGroups };
constexpr WideRefusal wide_served(uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0 || uint64_t{k} + r > kWideMaxShards) return WideRefusal::kShape;
  if ((k < r ? k : r) > kWideMaxRows) return WideRefusal::kRows;
  if (P < kVecMinP) return WideRefusal::kPacket;
  if (G == 0) return WideRefusal::kNoGroups;
  if (G >= (1ull << 32)) return WideRefusal::kGroups;
  return WideRefusal::kServed;
}
// A slot holds the largest wide record of the shape: 229,888 B at 224 + 32, so kPlanArenaBytes holds
// 291 groups per chunk there.
constexpr uint64_t wide_slot_stride(uint32_t k, uint32_t r) { return kWideHeader + uint64_t{k < r ? k : r} * k * 32u; }
// plan_arena with the wide slot: max(1, budget / stride) slots, at most G.
inline PlanArena wide_arena(uint32_t k, uint32_t r, uint64_t G, uint64_t budget) {
  const uint64_t stride = wide_slot_stride(k, r);
  uint64_t per = budget / stride;
  if (per == 0) per = 1;
  if (per > G) per = G;
  return {stride, per, per * stride};
}
// The workspace of a wide call, in the caller stream's stream_workspace: G record offsets, then the
// arena (plan_workspace without masks or symbol lengths of its own: the masks are the caller's).
inline PlanWorkspace wide_workspace(uint64_t G, const PlanArena& a) { return plan_workspace(G, false, false, a); }
// Row passes of a wide call's decode_wide per plan chunk.
constexpr uint32_t wide_passes(uint32_t k, uint32_t r) { return ((k < r ? k : r) + kWidePassRows - 1) / kWidePassRows; }
// The policy bits of decode_wide: those of the runtime-k decode_wave<0, 8> forms decode_form picks
// for the two layouts (in place; the recover's slots).
constexpr int kWidePolInPlace = kNtStore | kNoCoefBranch;
constexpr int kWidePolSlots = kNtStore | kNoCoefBranch | kCompactOut;
// One wide call (fec_wide.hip launch_decode_wide).
struct WideLaunch {
  const uint8_t* data;       // the data shards, only read when out != nullptr
  const uint8_t* parity;
  uint8_t* out;              // in place: the data shards again; slots: row (g, m) at (g * r + m) * P
  bool slots;                // the recover's layout
  const uint64_t* masks;     // four words per group, only read
  uint32_t* rec_off;         // workspace, one u32 per group
  uint8_t* status;           // nullable
  uint64_t groups;
  uint32_t k, r, P;
  PlanLaunch plan;           // arena, stride = wide_slot_stride, per_chunk, the r x k matrix
};

// ---- the wide address-table recover (fec_recover_scatter_wide_rs_dev; fec_wide_table.hip) ----
// The scatter recover's tables (TableRecoverLaunch) for a wide shape: k + r entries per group of
// addresses (0 = lost) and, nullable, lengths; k destinations per group.  The masks are derived
// from the addresses, four words per group, and the record builder reads them, so they always have
// a place: the caller's d_masks_out or the workspace.
struct WideTableLaunch {
  const uint64_t* addrs;     // groups * (k + r) absolute device addresses, 0 = lost
  const uint32_t* lens;      // nullable (NULL = every present shard has P): groups * (k + r)
  const uint64_t* dests;     // groups * k absolute device addresses, 0 = not wanted
  uint64_t groups;
  uint32_t k, r, P;
  uint8_t* status;           // nullable
  uint64_t* masks;           // written: four words per group, the caller's or the workspace's
  uint32_t* symlen;          // written when set: the caller's, else the workspace's when there is a
                             // length table (the kernel reads it), else nullptr
  uint32_t* rec_off;         // workspace, one u32 per group
  PlanLaunch plan;           // arena, stride = wide_slot_stride, per_chunk, the r x k matrix
};
// The policy bits of recover_scatter_wide: the table recovers' runtime-k form.
constexpr int kWideTablePol = kGatherPol | kNoCoefBranch;
// The workspace of a wide table call, byte offsets from its start, each region aligned as
// plan_workspace aligns its own: G record offsets; G masks of 32 B when the caller gives no
// d_masks_out; G symbol lengths when there is a length table and the caller asks for none; the
// arena (wide_arena), 256-B aligned.  A region not needed is empty.
inline PlanWorkspace wide_table_workspace(uint64_t G, bool masks_needed, bool symlen_needed, const PlanArena& a) {
  PlanWorkspace w{};
  w.rec_off = 0;
  w.masks = (G * sizeof(uint32_t) + 7u) & ~uint64_t{7};
  w.symlen = w.masks + (masks_needed ? G * 4u * sizeof(uint64_t) : 0);
  w.arena = (w.symlen + (symlen_needed ? G * sizeof(uint32_t) : 0) + 255u) & ~uint64_t{255};
  w.bytes = w.arena + a.bytes;
  return w;
}

// ---- the wide calls past the rows cap (fec_wide_rows_mode; fec_wide_deep.hip, fec_plan_build_deep.hpp) ----
// The cap of wide_served is the wide record builder's, not the code's: M is a scaled Cauchy matrix
// for every k + r <= 256.  A context in FEC_WIDE_ROWS_ALL serves the shapes past it with a builder
// that gives a whole workgroup one record (48.5 KiB of LDS, three workgroups per CU) and consumers
// that read a record whose erased ids lie elsewhere.  A shape wide_served serves takes the wide path
// in either mode; a shape past the cap takes the deep path for every group, whatever its e.
constexpr int kWideRowsCapped = 0, kWideRowsAll = 1;  // fec_hip.h FEC_WIDE_ROWS_CAPPED, FEC_WIDE_ROWS_ALL
constexpr bool wide_rows_mode_known(int mode) { return mode == kWideRowsCapped || mode == kWideRowsAll; }
constexpr uint32_t kWideDeepMaxRows = 128;  // min(k, r) with k + r <= 256; fec_plan_build_deep.hpp kDeepMaxE
// What the wide calls serve in FEC_WIDE_ROWS_ALL: wide_served without its rows cap.
constexpr WideRefusal wide_rows_all_served(uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0 || uint64_t{k} + r > kWideMaxShards) return WideRefusal::kShape;
  if (P < kVecMinP) return WideRefusal::kPacket;
  if (G == 0) return WideRefusal::kNoGroups;
  if (G >= (1ull << 32)) return WideRefusal::kGroups;
  return WideRefusal::kServed;
}
// The path of a wide call on a context in `mode`, decided here and nowhere else.
enum class WidePath : int { kRefused = 0, kWide, kDeep };
struct WideRoute {
  WidePath path;
  WideRefusal why;   // kServed unless refused
  uint32_t passes;   // consumer launches per plan chunk: wide_passes(k, r), up to 16 on the deep path
};
constexpr WideRoute wide_route(int mode, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  const WideRefusal capped = wide_served(G, k, r, P);
  if (capped == WideRefusal::kServed) return {WidePath::kWide, capped, wide_passes(k, r)};
  if (mode != kWideRowsAll) return {WidePath::kRefused, capped, 0};
  const WideRefusal all = wide_rows_all_served(G, k, r, P);
  if (all != WideRefusal::kServed) return {WidePath::kRefused, all, 0};
  return {WidePath::kDeep, all, wide_passes(k, r)};
}
// Form bit of the kernels that read a wide record (decode_wide, recover_scatter_wide): the record is
// a deep one, its erased ids where fec_plan_build_deep.hpp puts them.  Nothing else about the
// kernels differs, so the deep consumers are two more instantiations of the same templates.
constexpr int kDeepRecord = 16384;
constexpr int kWideDeepPolInPlace = kWidePolInPlace | kDeepRecord;
constexpr int kWideDeepTablePol = kWideTablePol | kDeepRecord;
// A slot holds the largest deep record of the shape, wide_slot_stride's formula past its cap:
// 524,800 B at 128 + 128, so kPlanArenaBytes holds 127 groups per chunk there.
constexpr uint64_t wide_deep_slot_stride(uint32_t k, uint32_t r) { return kWideHeader + uint64_t{k < r ? k : r} * k * 32u; }
// wide_arena with the deep slot.
inline PlanArena wide_deep_arena(uint32_t k, uint32_t r, uint64_t G, uint64_t budget) {
  const uint64_t stride = wide_deep_slot_stride(k, r);
  uint64_t per = budget / stride;
  if (per == 0) per = 1;
  if (per > G) per = G;
  return {stride, per, per * stride};
}

// ---- packed recover for every shape (fec_recover_packed_rs_dev, fec_recover_packed_wide_rs_dev;
// fec_packed.hip) ----
// The packed layout (fec_recover_batch_rs_dev_packed: group g's rows from row row_start[g], nothing
// between groups) for every shape a slot recover serves.  The row prefix writes row_start for every
// group; a record-addressed consumer then reads rec_off[g] and row_start[g] together and puts row
// m0 + m at out + (row_start[g] + m0 + m) * P.  A call the old packed call serves is handed to it.
//
// The paths of a call, decided here and nowhere else; the shim only launches.
enum class PackedPath : int {
  kRefused = 0,
  kEmpty,       // num_groups == 0 (one-word call): nothing launched, *total = 0
  kDelegate,    // what fec_recover_batch_rs_dev_packed serves: its forms (packed_form), untouched
  kCodebook,    // records from the dense codebook: rows prefix, classify, recover_packed
  kDevicePlan,  // past the codebook cap in FEC_PLAN_DEVICE: the same with build_records per plan chunk
  kWide,        // four-word masks: the wide prefix, classify_wide, per chunk build_records_wide, recover_packed_wide
  kDeep,        // the same past the wide builder's rows (FEC_WIDE_ROWS_ALL): build_records_deep
};
enum class PackedRefusal : int {
  kServed = 0,
  kShape,       // k = 0, r = 0 or k + r past the mask's width
  kRows,        // wide: min(k, r) > 32 on a context in FEC_WIDE_ROWS_CAPPED
  kPacket,      // packet_size < 16
  kNoGroups,    // wide: num_groups == 0
  kGroups,      // num_groups >= 2^32
  kRowIndex,    // num_groups * min(k, r) >= 2^32: row indices are 32-bit
  kNoCodebook,  // one-word: the codebook is past its cap and the context is in FEC_PLAN_CODEBOOK
};
struct PackedRoute {
  PackedPath path;
  PackedRefusal why;  // kServed unless refused
  uint32_t passes;    // consumer launches per (plan) chunk of the new consumers: ceil(min(k, r) / 8); else 0
};
// What the context's modes and the shape's codebook say, as bits.
constexpr int kPackedPlanDevice = 1;  // fec_decode_plan_mode is FEC_PLAN_DEVICE
constexpr int kPackedDense = 2;       // the shape's codebook of every pattern is inside its cap (gf256.hpp codebook_layout)
constexpr int kPackedRowsAll = 4;     // fec_wide_rows_mode is FEC_WIDE_ROWS_ALL
constexpr uint32_t kPackedMaxShards = 64;  // one-word masks (gf256.hpp kMaxDecodeShards)
// The policy bits of recover_packed and recover_packed_wide: the slot layout's runtime-k forms
// (decode_wave<0, 8> as decode_form picks it for compact_out; kWidePolSlots), 8 rows per pass.
constexpr int kPackedPol = kNtStore | kNoCoefBranch | kCompactOut;
constexpr uint32_t kPackedPassRows = 8;
constexpr uint32_t packed_passes(uint32_t k, uint32_t r) { return ((k < r ? k : r) + kPackedPassRows - 1) / kPackedPassRows; }
constexpr bool packed_rows_fit(uint64_t G, uint32_t k, uint32_t r) { return G * (k < r ? k : r) < (1ull << 32); }
// Whether fec_recover_batch_rs_dev_packed serves (G > 0, k, r, P): its own rule (decode_form of the
// compact-out call with device masks and a dense codebook, then packed_form) and its row-index limit.
inline bool packed_old_serves(uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0 || k + r > kPackedMaxShards || P == 0 || G * r >= (1ull << 32)) return false;
  const uint64_t some_mask = 0;
  DecodeLaunch a{};
  a.masks = &some_mask;  // not read: decode_form asks only whether there are masks
  a.compact_out = true;
  a.groups = G, a.k = k, a.r = r, a.P = P;
  return packed_form(a, decode_form(a), -1) != PackedForm::kRefused;
}
// fec_recover_packed_rs_dev.
inline PackedRoute packed_route(int bits, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0 || uint64_t{k} + r > kPackedMaxShards) return {PackedPath::kRefused, PackedRefusal::kShape, 0};
  if (P < kVecMinP) return {PackedPath::kRefused, PackedRefusal::kPacket, 0};
  if (G >= (1ull << 32)) return {PackedPath::kRefused, PackedRefusal::kGroups, 0};
  if (!packed_rows_fit(G, k, r)) return {PackedPath::kRefused, PackedRefusal::kRowIndex, 0};
  if (G == 0) return {PackedPath::kEmpty, PackedRefusal::kServed, 0};
  // (a shape the old call serves has a dense codebook: the mask-addressed shapes' books are a few KiB)
  if ((bits & kPackedDense) != 0 && packed_old_serves(G, k, r, P)) return {PackedPath::kDelegate, PackedRefusal::kServed, 0};
  if ((bits & kPackedDense) != 0) return {PackedPath::kCodebook, PackedRefusal::kServed, packed_passes(k, r)};
  if ((bits & kPackedPlanDevice) != 0) return {PackedPath::kDevicePlan, PackedRefusal::kServed, packed_passes(k, r)};
  return {PackedPath::kRefused, PackedRefusal::kNoCodebook, 0};
}
// fec_recover_packed_wide_rs_dev: wide_route's verdict, then the row-index limit.
inline PackedRoute packed_wide_route(int bits, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  const WideRoute w = wide_route((bits & kPackedRowsAll) != 0 ? kWideRowsAll : kWideRowsCapped, G, k, r, P);
  switch (w.why) {
    case WideRefusal::kServed: break;
    case WideRefusal::kShape: return {PackedPath::kRefused, PackedRefusal::kShape, 0};
    case WideRefusal::kRows: return {PackedPath::kRefused, PackedRefusal::kRows, 0};
    case WideRefusal::kPacket: return {PackedPath::kRefused, PackedRefusal::kPacket, 0};
    case WideRefusal::kNoGroups: return {PackedPath::kRefused, PackedRefusal::kNoGroups, 0};
    case WideRefusal::kGroups: return {PackedPath::kRefused, PackedRefusal::kGroups, 0};
  }
  if (!packed_rows_fit(G, k, r)) return {PackedPath::kRefused, PackedRefusal::kRowIndex, 0};
  return {w.path == WidePath::kDeep ? PackedPath::kDeep : PackedPath::kWide, PackedRefusal::kServed, w.passes};
}
// The record arena of a packed call on `path` of G groups: plan_arena, wide_arena or wide_deep_arena;
// none (all zero) on the codebook path, whose records are the codebook's.
inline PlanArena packed_arena(PackedPath path, uint32_t k, uint32_t r, uint64_t G, uint64_t budget) {
  switch (path) {
    case PackedPath::kDevicePlan: return plan_arena(k, r, G, budget);
    case PackedPath::kWide: return wide_arena(k, r, G, budget);
    case PackedPath::kDeep: return wide_deep_arena(k, r, G, budget);
    default: return {0, 0, 0};
  }
}
// The workspace of a packed call that takes a new consumer, byte offsets from its start, all of it
// ONE stream_workspace request (a second, larger request may synchronise and reallocate, which would
// leave the first pointer stale): the prefix's block sums, one u32 per kPackedRowsPerBlock groups; G
// record offsets; the record arena, 256-B aligned, empty on the codebook path.  The u32 arrays are
// 8-B aligned.
constexpr uint32_t kPackedRowsPerThread = 4;
constexpr uint32_t kPackedRowsPerBlock = 256 * kPackedRowsPerThread;  // fec_runs.hip kRowsPerBlock
// Blocks up to which every block of the row-start write adds up the sums before it itself (two
// launches); past it a one-block scan of the sums runs in between (fec_runs.hip kRowsDirectBlocks).
constexpr uint32_t kPackedRowsDirectBlocks = 4096;
struct PackedWorkspace {
  uint64_t block_sums, rec_off, arena, bytes;
};
inline PackedWorkspace packed_workspace(uint64_t G, const PlanArena& a) {
  PackedWorkspace w{};
  w.block_sums = 0;
  w.rec_off = ((G + kPackedRowsPerBlock - 1) / kPackedRowsPerBlock * sizeof(uint32_t) + 7u) & ~uint64_t{7};
  w.arena = (w.rec_off + G * sizeof(uint32_t) + 255u) & ~uint64_t{255};
  w.bytes = w.arena + a.bytes;
  return w;
}
// One packed call on a new consumer (fec_packed.hip launch_recover_packed).
struct PackedLaunch {
  PackedPath path;           // kCodebook, kDevicePlan, kWide or kDeep
  const uint8_t* data;       // the contiguous layouts, only read
  const uint8_t* parity;
  const uint64_t* masks;     // one word per group (kCodebook, kDevicePlan) or four, only read
  uint64_t groups;
  uint32_t k, r, P;
  uint8_t* out;              // packed rows
  uint32_t* row_start;       // one u32 per group, written for every group
  uint64_t* total;           // nullable
  uint8_t* status;           // nullable
  uint32_t* block_sums;      // workspace (packed_workspace)
  uint32_t* rec_off;         // workspace, one u32 per group
  const uint8_t* codebook;   // kCodebook: the dense CoefEntry codebook, device
  const uint64_t* binom;     // kCodebook, kDevicePlan: device, 65 x 65
  LevelMeta meta;            // kCodebook
  PlanLaunch plan;           // the other paths: arena (packed_arena), stride, per_chunk, the r x k matrix
};

// ---- the wide scatter encode (fec_encode_scatter_wide_rs_dev; fec_wide_encode.hip) ----
// The scatter encode's tables (TableEncodeLaunch) for groups of up to 256 shards: k entries per
// group of addresses (0 = absent) and, nullable, lengths; r destinations per group.  An encode
// builds no record, so the rows cap of wide_served (min(k, r) <= kWideMaxRows, the record
// builder's) is not its rule: 33 + 33, 128 + 128 and 1 + 255 are served.
struct WideEncodeLaunch {
  const uint64_t* addrs;     // groups * k absolute device addresses, 0 = absent (counts as zeros)
  const uint32_t* lens;      // nullable (NULL = every present packet has P): groups * k
  const uint64_t* dests;     // groups * r absolute device addresses, 0 = not wanted
  uint64_t groups;
  uint32_t k, r, P;
  uint32_t* symlen_out;      // nullable
  const void* tables;        // r x k CoefEntry, row 0 (all ones) included; not read when r == 1
};
// Whether the wide scatter encode serves (k, r, P, G), and if not, why: the one statement of that
// rule.
enum class WideEncodeRefusal : int { kServed = 0, kShape, kPacket, kNoGroups, kGroups };
constexpr WideEncodeRefusal wide_encode_served(uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0 || uint64_t{k} + r > kWideMaxShards) return WideEncodeRefusal::kShape;
  if (P < kVecMinP) return WideEncodeRefusal::kPacket;
  if (G == 0) return WideEncodeRefusal::kNoGroups;
  if (G >= (1ull << 32)) return WideEncodeRefusal::kGroups;
  return WideEncodeRefusal::kServed;
}
// The policy bits of encode_scatter_wide: recover_scatter_wide's (its rebuild is the same
// decode_piece<0, 8>, multiplying by every coefficient, row 0's ones included).
constexpr int kWideEncodePol = kWideTablePol;
struct WideEncodeForm {
  bool supported = false;  // false: the call is refused (wide_encode_served)
  uint32_t passes = 0;     // pass p: rows [p * pass_rows, min(r, (p + 1) * pass_rows))
  uint32_t pass_rows = 0;
  bool VAR = false;        // with a length table: loads masked by it
  bool xor_only = false;   // r == 1: the XOR of the packets, no coefficient table
  int POL = 0;
};
// The form the wide scatter encode runs for (k, r, P) with (var) or without a length table:
// ceil(r / 8) passes of encode_scatter_wide<POL, VAR>, every shape at runtime k.
inline WideEncodeForm wide_encode_form(uint32_t k, uint32_t r, uint32_t P, bool var) {
  WideEncodeForm f;
  if (wide_encode_served(1, k, r, P) != WideEncodeRefusal::kServed) return f;
  f.supported = true;
  f.pass_rows = kWidePassRows;
  f.passes = (r + kWidePassRows - 1) / kWidePassRows;
  f.VAR = var;
  f.xor_only = r == 1;
  f.POL = kWideEncodePol;
  return f;
}

// The passes of a runtime-k encode: at most kEncodePassRows parity rows per launch, pass p the rows
// [p * 8, min(r, p * 8 + 8)), the first pass owning the XOR row.  The rule of encode_v16<0, R> (the
// route the fixed-length gather encode takes for every shape but k=10 r=1) and of the table
// encodes.  QFEC_ENCODE_PASS_ROWS: the row counts a pass can have, X(extra..., R).
constexpr uint32_t kEncodePassRows = 8;
constexpr uint32_t encode_pass_rows(uint32_t r, uint32_t pass) {
  return r - pass * kEncodePassRows < kEncodePassRows ? r - pass * kEncodePassRows : kEncodePassRows;
}
#define QFEC_ENCODE_PASS_ROWS(X, ...)                                                               \
  X(__VA_ARGS__, 1) X(__VA_ARGS__, 2) X(__VA_ARGS__, 3) X(__VA_ARGS__, 4) X(__VA_ARGS__, 5) X(__VA_ARGS__, 6) \
  X(__VA_ARGS__, 7) X(__VA_ARGS__, 8)

// The table encodes, encode_gather_var<0, R, FIRST> and encode_scatter<0, R, FIRST, VAR>: every
// shape at runtime k in those passes, NT stores; the first pass also writes the symbol lengths.
constexpr int kTableEncodePol = kNtStore;
struct TableEncodeForm {
  bool supported = false;  // false: P < 16, the call is refused
  uint32_t passes = 0;     // pass p: encode_pass_rows(r, p) rows from row p * 8, FIRST = (p == 0)
  bool VAR = false;        // loads masked by the length table
};
// The form a table encode runs for (k, r, P) with (var) or without a length table.
inline TableEncodeForm table_encode_form(uint32_t /*k: every shape at runtime k*/, uint32_t r, uint32_t P, bool var) {
  TableEncodeForm f;
  if (P < kVecMinP) return f;
  f.supported = true;
  f.passes = (r + kEncodePassRows - 1) / kEncodePassRows;
  f.VAR = var;
  return f;
}
// The instantiations of encode_scatter, X(FIRST, VAR, R): every row count of a pass, as the first
// pass and as a later one (r = 8 + R), without and with the length table.
#define QFEC_SCATTER_ENCODE_FORMS(X)                                                  \
  QFEC_ENCODE_PASS_ROWS(X, true, false) QFEC_ENCODE_PASS_ROWS(X, false, false)       \
  QFEC_ENCODE_PASS_ROWS(X, true, true) QFEC_ENCODE_PASS_ROWS(X, false, true)

// ---- encode ----
enum class EncodeKernel : int { kBytes, kV16, kBits };

struct EncodeForm {
  EncodeKernel kernel;
  int K, R;       // template shape; K = 0: runtime k (the launcher's passes of up to 8 rows), R unused
  int OFF;        // OffsetKind of the instantiation
  int POL;
  uint32_t tile;  // groups per workgroup (encode_bits: per half), 0 = flat mapping
};

// Groups per workgroup of the tiled encodes (encode_bits: per half): pick_tile (the test
// library's TestKnob::kEncodeTile overrides it when the tile fits 512 lanes).
inline uint32_t encode_tile(const EncodeLaunch& a) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  const long tile_env = test_knob(TestKnob::kEncodeTile, 0);
  return tile_env > 0 && cpp > 0 && uint32_t(tile_env) * cpp <= 512 ? uint32_t(tile_env) : pick_tile(cpp, a.k, a.P);
}

// Bit-sliced encode for a compile-time shape where it is faster than the tables (r >= 4: the
// table form is VALU-bound there); the test library's TestKnob::kEncodeBits forces it on (1,
// every compiled shape) or off (0).
inline bool use_encode_bits(uint32_t r) {
  const long mode = test_knob(TestKnob::kEncodeBits, -1);
  return mode == 1 || (mode < 0 && r >= 4);
}

// kStageRows for a launch whose workgroup window (groups_per_block * r * P bytes) fits the LDS a
// workgroup may take (the test library's TestKnob::kEncodeStage: 1 on, 0 off).  A flat launch
// (P > 8192, groups_per_block 0) passes too: it runs the kStageRows instantiation, whose kernel
// stages only when tiled and otherwise stores directly.
inline bool use_stage_rows(const EncodeLaunch& a, uint32_t groups_per_block) {
  const long mode = test_knob(TestKnob::kEncodeStage, kEncodeStageDefault);
  return mode == 1 && a.P % 16 == 0 && uint64_t(groups_per_block) * a.r * a.P <= 64u * 1024u;
}

// The form launch_encode(a) runs.
inline EncodeForm encode_form(const EncodeLaunch& a) {
  EncodeForm f{EncodeKernel::kBytes, 0, 0, static_cast<int>(a.off_kind), 0, 0};
  if (a.P < kVecMinP) return f;
  f.kernel = EncodeKernel::kV16, f.POL = kNtStore, f.tile = encode_tile(a);
  const auto shape = [&a](uint32_t k, uint32_t r) { return a.k == k && a.r == r; };
  const auto pick = [&f, &a](int pol) {
    f.K = static_cast<int>(a.k), f.R = static_cast<int>(a.r), f.POL = pol;
    return f;
  };
  // A compile-time encode in its staged form (kStageRows) where the workgroup's window fits
  // (use_stage_rows), else with POL's direct stores.
  const auto staged = [&a](uint32_t groups_per_block) { return use_stage_rows(a, groups_per_block) ? kStageRows : 0; };
  if (a.off_kind == OffsetKind::kNone) {
    // The paired-coefficient arithmetic (kPairMac): +0.9% at k=20 r=5 (5.53 vs 5.58 ms),
    // +1.0% at k=10 r=3 (2.65 vs 2.68 ms), same box, alternating runs
    // (profiles/r02_ab_encode_pair.txt).  Staged rows keep the default cache policy, NT stores
    // with cached loads (C2 2.590 ms vs 2.606-2.702, C4 4.991 vs 5.062-5.345 for the other
    // three; profiles/r05k/sweep_mempol.jsonl).
    // Bit-sliced form (bitslice.hpp) while a workgroup holds whole groups.  k=20 r=5 (VALU-
    // bound with the tables): 5.24-5.41 vs 5.37-5.54 ms over six boxes; k=10 r=3 (HBM-bound
    // with the tables) 2.74-2.76 vs 2.63-2.66 ms, so not chosen there.  4 packets in flight per
    // lane (2: 5.70 ms, 8: 5.28, 20: 5.91-6.03; profiles/r03_ab_bits.txt).
    if (a.P <= 8192 && use_encode_bits(a.r) && (shape(20, 5) || shape(10, 3))) {
      f.kernel = EncodeKernel::kBits;
      return pick(kNtStore | staged(2 * f.tile));
    }
    if (shape(10, 3)) return pick(kNtStore | kPairMac | staged(f.tile));
    // staged rows measured per shape (scripts/ab_stage_rows.py, profiles/r05k): k=10 r=1 level
    // (2.383 vs 2.378 ms), k=10 r=2 -1.5% (2.537 vs 2.575), k=4 r=2 +8.9% (1.351 vs 1.241): the
    // XOR row and k=4 keep their direct stores
    if (shape(10, 1) || shape(4, 2)) return pick(kNtStore);
    if (shape(20, 5)) return pick(kNtStore | kPairMac);
    // k=10 r=2 (the campaign's 20% FEC rate): compile-time k (2.50 vs 2.56 ms for the runtime-k
    // loop, profiles/r02_ab_encode_r1r2_defaults.txt)
    if (shape(10, 2)) return pick(kNtStore | kPairMac | staged(f.tile));
  } else if ((a.off_kind == OffsetKind::kU32 || a.off_kind == OffsetKind::kAddr) && shape(10, 1)) {
    return pick(kNtStore);  // the legacy call's and the coalescer's instantiations
  }
  return f;  // runtime k
}

}  // namespace qfec
