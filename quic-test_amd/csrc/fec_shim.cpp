// fec_shim.cpp — C-ABI of libfec_hip.so (include/fec_xor_simd.h, include/fec_hip.h).
//
// Replaces the reference's native library internal/fec/fec_xor_simd.cpp behind the
// same eleven symbols, and adds the batch GF(2^8) encode/decode API.  All arithmetic
// runs in the gfx950 kernels (fec_kernels.hpp names their units); this file owns contexts, device
// buffers, host<->device staging, per-(k,r) plans and error reporting.
//
// Threading (SURVEY.md §8(b) "Threading"): one context per caller stream of work; every
// entry point locks its context and binds the context's device for the duration of the
// call (Go goroutines migrate between OS threads and the HIP current device is
// thread-local), restoring the caller's device afterwards.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "fec_hip.h"
#include "fec_internal.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_routes.hpp"
#include "gf256.hpp"

using qfec::classify_ptr;
using qfec::kPipeSlots;
using qfec::Mem;

#define QFEC_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

int hip_fail(hipError_t e, const char* what) {
  set_error("%s: %s", what, hipGetErrorString(e));
  return FEC_ERR_HIP;
}

#define QFEC_HIP(call)                                 \
  do {                                                 \
    const hipError_t qfec_e_ = (call);                 \
    if (qfec_e_ != hipSuccess) return hip_fail(qfec_e_, #call); \
  } while (0)

// Binds a device for the scope, restores the caller's device on exit.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
    if (!ok) (void)hipGetLastError();
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Grow-only device buffer (freed with its owner).
struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (ptr) {
      (void)hipFree(ptr);
      ptr = nullptr;
      cap = 0;
    }
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&ptr, want);
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
};

struct EncodePlan {
  DevBuf tables;  // (r-1) * k CoefEntry
};

struct DecodePlan {
  bool dense = false;          // dense codebook of every pattern (else: sparse per call)
  qfec::CodebookLayout layout;
  DevBuf codebook;
  qfec::CodebookLayout clayout;  // compact (coefficient-byte) book, built on first use
  DevBuf cbook;
  std::vector<uint8_t> M;      // parity matrix, for sparse per-call records
  DevBuf sparse_book;          // the last sparse call's records
  DevBuf d_matrix;             // M on the device, for records built there (FEC_PLAN_DEVICE); on first use
};

constexpr uint64_t kCodebookCap = 2ull << 30;  // 2 GiB of recovery tables per (k, r)

// Grow-only page-locked host buffer (staging for the compacted host decode).
struct HostBuf {
  void* ptr = nullptr;
  void* dev = nullptr;   // the same memory as the kernels address it
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    const size_t want = bytes < 4096 ? 4096 : bytes;
    const hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    cap = want;
    if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess || dev == nullptr) {
      (void)hipGetLastError();
      dev = ptr;  // unified addressing: the host pointer is the device address
    }
    return hipSuccess;
  }
  void release() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    dev = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
  template <class T>
  T* dev_as() const { return static_cast<T*>(dev); }
};

// Host threads for the CPU side of the host-resident paths (gathering / scattering
// packets): QUICFEC_HOST_THREADS, default 8, at most the machine's.
unsigned host_threads() {
  static const unsigned n = [] {
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    unsigned want = 8;
    if (const char* v = std::getenv("QUICFEC_HOST_THREADS")) {
      const int x = std::atoi(v);
      if (x > 0) want = static_cast<unsigned>(x);
    }
    return want < hw ? want : hw;
  }();
  return n;
}

// f(begin, end) over [0, n) split across host_threads() threads (inline when small).
template <class F>
void parallel_for(uint64_t n, uint64_t min_per_thread, F&& f) {
  uint64_t nt = host_threads();
  if (min_per_thread > 0 && n / min_per_thread < nt) nt = n / min_per_thread;
  if (nt <= 1) {
    f(uint64_t(0), n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt - 1);
  for (uint64_t t = 1; t < nt; ++t) th.emplace_back([&f, n, nt, t] { f(n * t / nt, n * (t + 1) / nt); });
  f(uint64_t(0), n / nt);
  for (auto& x : th) x.join();
}

// Page-locked buffers this library handed out (fec_alloc_slab / _numa / fec_alloc_repair_buffer).
// The Go wrapper passes the same two of them to every legacy call (fec_cgo.go:64, :76, :138);
// finding them here keeps hipPointerGetAttributes -- a runtime lock and a lookup per pointer --
// off the per-call path.
struct PinnedRange {
  uintptr_t hi;   // one past the last byte
  uintptr_t dev;  // device address of the first byte
};
std::shared_mutex g_pin_mu;
std::map<uintptr_t, PinnedRange> g_pinned;  // by first byte

void pinned_register(void* p, size_t len) {
  if (!p || len == 0) return;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || d == nullptr) {
    (void)hipGetLastError();
    d = p;
  }
  std::unique_lock<std::shared_mutex> lk(g_pin_mu);
  g_pinned[reinterpret_cast<uintptr_t>(p)] = PinnedRange{reinterpret_cast<uintptr_t>(p) + len, reinterpret_cast<uintptr_t>(d)};
}

void pinned_unregister(void* p) {
  std::unique_lock<std::shared_mutex> lk(g_pin_mu);
  g_pinned.erase(reinterpret_cast<uintptr_t>(p));
}

bool pinned_lookup(const void* p, void** dev) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  std::shared_lock<std::shared_mutex> lk(g_pin_mu);
  auto it = g_pinned.upper_bound(a);
  if (it == g_pinned.begin()) return false;
  --it;
  if (a >= it->second.hi) return false;
  if (dev) *dev = reinterpret_cast<void*>(it->second.dev + (a - it->first));
  return true;
}

}  // namespace

// fec_internal.hpp (the coalescer classifies its callers' buffers too)
Mem qfec::classify_ptr(const void* p, void** dev) {
  if (dev) *dev = nullptr;
  if (!p) return Mem::kHost;
  if (pinned_lookup(p, dev)) return Mem::kPinned;
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return Mem::kHost;
  }
  if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) return Mem::kDevice;
  if (attr.type == hipMemoryTypeHost) {
    if (dev) *dev = attr.devicePointer ? attr.devicePointer : const_cast<void*>(p);
    return Mem::kPinned;
  }
  return Mem::kHost;
}

namespace {

// Completion wait of the zero-copy calls.  The runtime's blocking wait: polling
// hipStreamQuery from the calling thread measured slower (one group: 20 vs 15.5 us;
// profiles/r01_latency_sweep.txt).
hipError_t wait_stream(hipStream_t s) { return hipStreamSynchronize(s); }

// The zero-copy limits of this call (fec_routes.hpp); QUICFEC_SMALL_CALL_BYTES overrides both.
qfec::SmallCallLimits small_call_limits() {  // read per call: tests switch paths in one process
  const char* v = std::getenv("QUICFEC_SMALL_CALL_BYTES");
  return qfec::small_call_limits(v && *v ? std::atoll(v) : -1);
}

}  // namespace

// One stage of the host<->device pipeline: its own stream and device buffers.
struct PipeSlot {
  hipStream_t s = nullptr;
  DevBuf in, par, mask, status, rec;
  HostBuf h_in, h_par, h_mask;          // compacted host decode staging
  std::vector<uint64_t> h_groups;        // the groups gathered into this slot's staging
};

// QUICFEC_PIPE_CHUNK_BYTES overrides the chunk size (tests use small chunks to run many).
uint64_t pipe_chunk_bytes() {
  const char* v = std::getenv("QUICFEC_PIPE_CHUNK_BYTES");
  const long long x = v ? std::atoll(v) : 0;
  return x > 0 ? static_cast<uint64_t>(x) : qfec::kPipeChunkBytes;
}

// A caller stream's decode workspace (stream_workspace).
struct StreamWorkspace {
  hipStream_t s = nullptr;
  DevBuf buf;
  uint64_t last_use = 0;
  // one-launch packed recover (recover_runs): ticket, chunk totals and look-back words, zeroed
  // when allocated; `epoch` = the last look-back epoch a launch on this stream used
  DevBuf runs;
  uint32_t epoch = 0;
};

struct FECEncoderCtx {
  double redundancy = 0.10;
  uint32_t max_groups = 1024;
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // staging / workspace buffers
  DevBuf d_in, d_off, d_out, d_mask, d_status, d_binom;
  HostBuf z_in, z_out, z_aux;           // zero-copy staging of small host-resident calls
  PipeSlot pipe[kPipeSlots];
  std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<EncodePlan>> enc_plans;
  std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<DecodePlan>> dec_plans;
  // the r x k parity matrix on the device, one per shape the wide calls met (wide_call)
  std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<DevBuf>> wide_matrices;
  // the r x k coefficient table, row 0 included, one per shape the wide scatter encode met
  // (wide_encode_tables), beside enc_plans' (r - 1) x k tables
  std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<DevBuf>> wide_enc_tables;
  // Message of the last failing call on this context (fec_ctx_last_error): callers whose
  // threads migrate between the failing call and the read (Go goroutines) cannot rely on the
  // thread-local fec_hip_last_error.  Own lock: readable while a call holds `mu`.
  std::mutex err_mu;
  std::string last_error;
  // fec_decode_loss_hint: expected share of groups with lost data in device-resident decode
  // calls (< 0: unknown, treated as dense).
  double decode_need_share = -1.0;
  // fec_decode_plan_mode: where the device-resident calls take the records of a shape without a
  // dense codebook from
  int plan_mode = FEC_PLAN_CODEBOOK;
  // fec_wide_rows_mode: whether the wide decoders serve the shapes past min(k, r) <= 32
  int wide_rows_mode = FEC_WIDE_ROWS_CAPPED;
  // per-stream record-offset workspaces of the device-resident decodes (stream_workspace)
  std::vector<std::unique_ptr<StreamWorkspace>> stream_ws;
  uint64_t ws_clock = 0;
  // a call took a caller's stream (pick_stream): its kernels may still be queued there when the
  // context is freed, reading the plans' tables and the workspaces
  bool caller_streams = false;

  ~FECEncoderCtx() {
    DeviceGuard g(device);
    // Freeing waits for the calls queued on caller streams (include/fec_hip.h): their streams are
    // not known here any more (or gone), so the device drains.  Also the mask-addressed decodes
    // and the encodes, which take no workspace but read the plan's codebook and tables.
    if (caller_streams || !stream_ws.empty()) (void)hipDeviceSynchronize();
    stream_ws.clear();
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& p : pipe)
      if (p.s) (void)hipStreamSynchronize(p.s);
    d_in.release();
    d_off.release();
    d_out.release();
    d_mask.release();
    d_status.release();
    d_binom.release();
    z_in.release();
    z_out.release();
    z_aux.release();
    for (auto& p : pipe) {
      p.in.release();
      p.par.release();
      p.mask.release();
      p.status.release();
      p.rec.release();
      p.h_in.release();
      p.h_par.release();
      p.h_mask.release();
      if (p.s) (void)hipStreamDestroy(p.s);
    }
    enc_plans.clear();
    dec_plans.clear();
    wide_matrices.clear();
    wide_enc_tables.clear();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

// What every exported call that returns a code is wrapped in: the thread's message cleared, f()
// run, and a non-zero code's message copied into the context (fec_ctx_last_error).
template <class F>
int api_call(FECEncoderCtx* ctx, F&& f) {
  g_last_error.clear();
  const int rc = f();
  if (rc != FEC_OK && ctx != nullptr) {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    ctx->last_error = g_last_error.empty() ? "error code " + std::to_string(rc) : g_last_error;
  }
  return rc;
}

// The context locked and its device bound for the scope.  rc: FEC_OK, or FEC_ERR_NODEV when the
// device could not be bound -- with the message "<what>: cannot bind device N" for the calls that
// name themselves, with none for the others.
struct CtxBound {
  std::lock_guard<std::mutex> lk;
  DeviceGuard dg;
  int rc = FEC_OK;
  explicit CtxBound(FECEncoderCtx* ctx, const char* what = nullptr) : lk(ctx->mu), dg(ctx->device) {
    if (dg.ok) return;
    if (what) set_error("%s: cannot bind device %d", what, ctx->device);
    rc = FEC_ERR_NODEV;
  }
};

// The first use of a kernel on a device loads its translation unit's code object there, and the
// resident encoder's first call allocates its page-locked ring: together ~26 ms that otherwise
// land on the first fec_encode_batch of the process — the first repair packet of the first QUIC
// stream (batcher_latency legacy_raw: max delay 25.8-27.5 ms without, 11.5-12.2 ms with the code
// objects loaded here).  Loaded here: the six units of the contiguous calls (fec_kernels.hpp
// load_kernel_units: the encodes, the decodes, decode_fused, the packed rows, the resident server,
// the utilities), so none of their first calls loads one; then one launch of the fill kernel, the
// device's first.  The address-table and plan units load at their first call.  Done once per
// device, at the first context; failures are left to the calls that follow (they report them).
void warm_device_once(int device, hipStream_t s) {
  constexpr int kMaxWarm = 64;
  static std::once_flag once[kMaxWarm];
  if (device < 0 || device >= kMaxWarm || std::getenv("QUICFEC_NO_WARMUP") != nullptr) return;
  std::call_once(once[device], [&] {
    (void)qfec::load_kernel_units();
    uint8_t* p = nullptr;
    if (hipMalloc(&p, 256) == hipSuccess) {
      if (qfec::launch_fill_splitmix(p, 256, 0, 0, s) == hipSuccess) (void)hipStreamSynchronize(s);
      (void)hipFree(p);
    }
    (void)hipGetLastError();
    qfec::coalesce_prepare(device);
  });
}

FECEncoderCtx* make_ctx(double redundancy, uint32_t max_groups, int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("fec_encoder_new: no HIP device available");
    return nullptr;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= n) {
    set_error("fec_encoder_new: device %d out of range (%d devices)", device, n);
    return nullptr;
  }
  DeviceGuard g(device);
  if (!g.ok) {
    set_error("fec_encoder_new: hipSetDevice(%d) failed", device);
    return nullptr;
  }
  auto* ctx = new FECEncoderCtx();
  // fec_xor_simd.cpp:540-541 defaults
  ctx->redundancy = (redundancy > 0 && redundancy <= 1.0) ? redundancy : 0.10;
  ctx->max_groups = max_groups > 0 ? max_groups : 1024;
  ctx->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);
  if (e != hipSuccess) {
    set_error("fec_encoder_new: hipStreamCreate: %s", hipGetErrorString(e));
    ctx->stream = nullptr;
    delete ctx;
    return nullptr;
  }
  warm_device_once(device, ctx->stream);
  return ctx;
}

int get_encode_plan(FECEncoderCtx* ctx, uint32_t k, uint32_t r, const void** tables) {
  if (r == 1) {  // the XOR row alone needs no coefficients, so any number of packets works
    *tables = nullptr;
    return k > 0 ? FEC_OK : FEC_ERR_RANGE;
  }
  auto key = std::make_pair(k, r);
  auto it = ctx->enc_plans.find(key);
  if (it == ctx->enc_plans.end()) {
    std::vector<uint8_t> M;
    if (!qfec::parity_matrix(k, r, M)) {
      set_error("encode: unsupported k=%u r=%u (need k>0, r>0, k+r<=256)", k, r);
      return FEC_ERR_RANGE;
    }
    auto plan = std::make_unique<EncodePlan>();
    if (r > 1) {
      std::vector<qfec::CoefEntry> tab(size_t(r - 1) * k);
      for (uint32_t i = 1; i < r; ++i)
        for (uint32_t j = 0; j < k; ++j) tab[(i - 1) * k + j] = qfec::make_entry(M[i * k + j]);
      QFEC_HIP(plan->tables.ensure(tab.size() * sizeof(qfec::CoefEntry)));
      QFEC_HIP(hipMemcpy(plan->tables.ptr, tab.data(), tab.size() * sizeof(qfec::CoefEntry),
                         hipMemcpyHostToDevice));
    }
    it = ctx->enc_plans.emplace(key, std::move(plan)).first;
  }
  *tables = it->second->tables.ptr;
  return FEC_OK;
}

int get_decode_plan(FECEncoderCtx* ctx, uint32_t k, uint32_t r, DecodePlan** out) {
  auto key = std::make_pair(k, r);
  auto it = ctx->dec_plans.find(key);
  if (it == ctx->dec_plans.end()) {
    auto plan = std::make_unique<DecodePlan>();
    if (k + r > qfec::kMaxDecodeShards || !qfec::parity_matrix(k, r, plan->M)) {
      set_error("decode: unsupported k=%u r=%u (need k+r<=64)", k, r);
      return FEC_ERR_RANGE;
    }
    // Dense codebook when it fits the cap; otherwise records are built per call for the
    // patterns present (build_sparse_plan).
    plan->dense = qfec::codebook_layout(k, r, kCodebookCap, plan->layout);
    if (plan->dense) {
      std::vector<uint8_t> book;
      if (!qfec::build_codebook(plan->layout, plan->M, book)) {
        set_error("decode: singular recovery submatrix for k=%u r=%u", k, r);
        return FEC_ERR_RANGE;
      }
      QFEC_HIP(plan->codebook.ensure(book.size()));
      QFEC_HIP(hipMemcpy(plan->codebook.ptr, book.data(), book.size(), hipMemcpyHostToDevice));
    }
    if (!ctx->d_binom.ptr) {
      QFEC_HIP(ctx->d_binom.ensure(sizeof(qfec::binom().c)));
      QFEC_HIP(hipMemcpy(ctx->d_binom.ptr, qfec::binom().c, sizeof(qfec::binom().c),
                         hipMemcpyHostToDevice));
    }
    it = ctx->dec_plans.emplace(key, std::move(plan)).first;
  }
  *out = it->second.get();
  return FEC_OK;
}

// Caller holds ctx->mu.
hipStream_t pick_stream(FECEncoderCtx* ctx, void* stream) {
  if (stream) ctx->caller_streams = true;
  return stream ? static_cast<hipStream_t>(stream) : ctx->stream;
}

// Device-resident encode, contiguous layout.  Caller holds ctx->mu and the device.
int encode_dev_locked(FECEncoderCtx* ctx, const uint8_t* d_data, const void* d_offsets,
                      qfec::OffsetKind ok, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                      uint8_t* d_parity, hipStream_t s) {
  const void* tables = nullptr;
  int rc = get_encode_plan(ctx, k, r, &tables);
  if (rc != FEC_OK) return rc;
  qfec::EncodeLaunch a;
  a.data = d_data;
  a.offsets = d_offsets;
  a.off_kind = ok;
  a.parity = d_parity;
  a.groups = G;
  a.k = k;
  a.r = r;
  a.P = P;
  a.tables = tables;
  QFEC_HIP(qfec::launch_encode(a, s));
  return FEC_OK;
}

// Record-offset workspace of device-resident decodes, one buffer per caller stream: calls
// on one stream run in stream order, so the next call on it may reuse the buffer while the
// previous call's kernels are still queued; decodes in flight on different streams never
// share one (the context-wide buffer they used to share could be overwritten by the next
// call's classify before the previous call's decode read it).  A buffer grows only after
// its stream has drained; the least recently used of kMaxStreamWorkspaces is dropped after
// a device synchronize.  (A per-call stream-ordered allocation, hipMallocAsync/hipFreeAsync,
// handed out memory that a queued decode on the same stream was still reading:
// tools/batcher_latency.cpp decode mode, ~20% of k=10 r=2 groups wrong.)  Caller holds
// ctx->mu.
constexpr size_t kMaxStreamWorkspaces = 16;

hipError_t find_stream_ws(FECEncoderCtx* ctx, hipStream_t s, StreamWorkspace** out);

hipError_t stream_workspace(FECEncoderCtx* ctx, hipStream_t s, size_t bytes, void** out) {
  StreamWorkspace* w = nullptr;
  const hipError_t fe = find_stream_ws(ctx, s, &w);
  if (fe != hipSuccess) return fe;
  if (bytes > w->buf.cap) {
    if (w->buf.ptr) {
      const hipError_t e = hipStreamSynchronize(s);  // queued calls may still read the old one
      if (e != hipSuccess) return e;
    }
    const hipError_t e = w->buf.ensure(bytes);
    if (e != hipSuccess) return e;
  }
  *out = w->buf.ptr;
  return hipSuccess;
}

// The recover_runs workspace of caller stream s and the first look-back epoch of a call of G
// groups.  Epochs are never reused while the buffer lives (words of earlier launches on this
// stream cannot match); the buffer is zeroed when allocated and when the epochs wrap (on the
// stream, so after the launches already queued on it).
hipError_t runs_workspace(FECEncoderCtx* ctx, hipStream_t s, uint64_t G, void** out, uint32_t* epoch) {
  StreamWorkspace* w = nullptr;
  hipError_t e = find_stream_ws(ctx, s, &w);
  if (e != hipSuccess) return e;
  const uint64_t bytes = qfec::runs_workspace_bytes(G);
  const uint32_t n = qfec::runs_launches(G);
  const long lim = qfec::test_knob(qfec::TestKnob::kRunsEpochLimit, qfec::kRunsEpochLimit);
  const uint32_t limit = lim >= 2 && lim < static_cast<long>(qfec::kRunsEpochLimit) ? static_cast<uint32_t>(lim)
                                                                                     : qfec::kRunsEpochLimit;
  if (n >= limit) return hipErrorInvalidValue;  // never at 2^30: a call has at most 2^32 / 512 launches
  bool fresh = false;
  if (bytes > w->runs.cap) {
    if (w->runs.ptr && (e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if ((e = w->runs.ensure(bytes)) != hipSuccess) return e;
    w->epoch = 0;
    fresh = true;
  }
  // the epoch accounting (fec_forms.hpp runs_epochs; tests/csrc/runs_epoch_test.cpp)
  const qfec::RunsEpochs ep = qfec::runs_epochs(w->epoch, n, limit);
  if (fresh || ep.rezero) {
    if ((e = hipMemsetAsync(w->runs.ptr, 0, w->runs.cap, s)) != hipSuccess) return e;
    if (!fresh) {  // the wrap alone is traced (test library): not the first allocation, not growth
      qfec::LaunchRecord t;
      t.form = static_cast<int64_t>(qfec::LaunchForm::kRunsRezero);
      t.items = static_cast<int64_t>(w->runs.cap);  // bytes zeroed
      t.aux = static_cast<int64_t>(w->epoch);       // the last epoch used before the wrap
      qfec::trace_launch(t);
    }
  }
  *out = w->runs.ptr;
  *epoch = ep.first;
  w->epoch = ep.first + n - 1;
  return hipSuccess;
}

hipError_t find_stream_ws(FECEncoderCtx* ctx, hipStream_t s, StreamWorkspace** out) {
  StreamWorkspace* w = nullptr;
  for (auto& e : ctx->stream_ws)
    if (e->s == s) {
      w = e.get();
      break;
    }
  if (!w) {
    if (ctx->stream_ws.size() >= kMaxStreamWorkspaces) {
      auto lru = std::min_element(ctx->stream_ws.begin(), ctx->stream_ws.end(),
                                  [](const auto& x, const auto& y) { return x->last_use < y->last_use; });
      const hipError_t e = hipDeviceSynchronize();  // its stream may be gone: drain everything
      if (e != hipSuccess) return e;
      ctx->stream_ws.erase(lru);
    }
    ctx->stream_ws.push_back(std::make_unique<StreamWorkspace>());
    w = ctx->stream_ws.back().get();
    w->s = s;
  }
  w->last_use = ++ctx->ws_clock;
  *out = w;
  return hipSuccess;
}

// The codebook's levels e = 1..32 as the classify rule reads them (fec_device.hpp classify_mask).
qfec::LevelMeta level_meta(const qfec::CodebookLayout& layout, uint32_t r) {
  qfec::LevelMeta m{};
  for (uint32_t e = 1; e <= 32; ++e) {
    m.base[e] = layout.level_base[e];
    m.stride[e] = layout.level_stride[e];
    m.count_r[e] = qfec::binom().c[r][e];
  }
  return m;
}

// One device-resident decode, contiguous layout (decode_dev_locked).  Every pointer is a device
// address (of device memory, or of page-locked host memory for the zero-copy calls).
struct DecodeCall {
  uint8_t* data = nullptr;         // the data shards; rebuilt in place unless `out` is set
  const uint8_t* parity = nullptr;
  const uint64_t* masks = nullptr;
  struct { uint64_t G; uint32_t k, r, P; } shape{};
  uint8_t* status = nullptr;       // nullable
  hipStream_t stream = nullptr;
  DevBuf* rec = nullptr;           // a pipeline slot's record-offset buffer; NULL: the stream's workspace
  uint8_t* out = nullptr;          // where rebuilt shards are stored; NULL: in place in `data`
  double need_share = -1.0;        // share of groups to rebuild, from a host scan; < 0: the context's hint
  bool compact_out = false;        // rebuilt rows one run per group, `data` only read (DecodeLaunch)
  uint32_t* row_start = nullptr;   // set: packed rows (fec_recover_batch_rs_dev_packed), written
  uint64_t* row_total = nullptr;   //   with them, nullable: all rows
  bool device_masks = false;       // a device-resident call (the masks are the caller's device memory): in
                                   // FEC_PLAN_DEVICE a shape without a dense codebook has its records built there
};

// The parity matrix of a plan on the device, for build_records (uploaded once per plan).
int plan_matrix(DecodePlan* plan, const uint8_t** out) {
  if (!plan->d_matrix.ptr) {
    QFEC_HIP(plan->d_matrix.ensure(plan->M.size()));
    QFEC_HIP(hipMemcpy(plan->d_matrix.ptr, plan->M.data(), plan->M.size(), hipMemcpyHostToDevice));
  }
  *out = plan->d_matrix.as<uint8_t>();
  return FEC_OK;
}

// The workspace of a device-plan call of G groups on caller stream s (fec_forms.hpp plan_arena,
// plan_workspace) and its launch description.
int plan_workspace_locked(FECEncoderCtx* ctx, DecodePlan* plan, hipStream_t s, uint64_t G, uint32_t k, uint32_t r,
                          bool own_masks, bool own_symlen, qfec::PlanWorkspace* w, uint8_t** ws, qfec::PlanLaunch* p) {
  const qfec::PlanArena arena = qfec::plan_arena(k, r, G, qfec::plan_arena_budget());
  *w = qfec::plan_workspace(G, own_masks, own_symlen, arena);
  int rc = plan_matrix(plan, &p->matrix);
  if (rc != FEC_OK) return rc;
  void* base = nullptr;
  QFEC_HIP(stream_workspace(ctx, s, w->bytes, &base));
  *ws = static_cast<uint8_t*>(base);
  p->arena = *ws + w->arena;
  p->stride = arena.stride;
  p->per_chunk = arena.per_chunk;
  return FEC_OK;
}

// Caller holds ctx->mu and the device.
int decode_dev_locked(FECEncoderCtx* ctx, const DecodeCall& c) {
  // under the names the failure messages below quote (QFEC_HIP reports the failing expression)
  const auto [G, k, r, P] = c.shape;
  const uint64_t* const d_masks = c.masks;
  uint8_t *const d_status = c.status, *const d_out = c.out;
  DevBuf* const rec = c.rec;
  uint32_t* const row_start = c.row_start;
  uint64_t* const row_total = c.row_total;
  const hipStream_t s = c.stream;
  DecodePlan* plan = nullptr;
  int rc = get_decode_plan(ctx, k, r, &plan);
  if (rc != FEC_OK) return rc;
  qfec::DecodeLaunch a;
  a.data = c.data;
  a.parity = c.parity;
  a.masks = d_masks;
  a.rec_off = nullptr;
  a.out = d_out;
  a.compact_out = c.compact_out;
  a.status = d_status;
  a.codebook = plan->codebook.as<uint8_t>();
  a.binom = ctx->d_binom.as<uint64_t>();
  a.meta = level_meta(plan->layout, r);
  a.groups = G;
  a.k = k;
  a.r = r;
  a.P = P;
  a.rec_ready = !plan->dense;
  // Groups per wave of the mask-addressed form: the scan form when the caller knows that
  // few groups need a rebuild (need_share, from a host scan of the masks); device-resident
  // callers get one wave per group (the test library's TestKnob::kDecodeScan overrides it).
  const double need_share = c.need_share < 0.0 ? ctx->decode_need_share : c.need_share;
  if (need_share >= 0.0 && need_share < qfec::kDecodeScanMaxShare) a.scan = qfec::kDecodeScanGroups;
  a.scan = static_cast<uint32_t>(qfec::test_knob(qfec::TestKnob::kDecodeScan, a.scan));
  // The kernel form of this call (fec_forms.hpp); what is attached to `a` below -- codebook,
  // workspace, row starts -- does not change it.
  const qfec::DecodeForm form = qfec::decode_form(a);
  if (form.compact_tables) {
    // the form reads bare coefficient bytes: the compact book of the same patterns
    if (!plan->cbook.ptr) {
      std::vector<uint8_t> book;
      if (!qfec::codebook_layout(k, r, kCodebookCap, plan->clayout, /*compact=*/true) ||
          !qfec::build_codebook(plan->clayout, plan->M, book)) {
        set_error("decode: compact codebook failed for k=%u r=%u", k, r);
        return FEC_ERR_RANGE;
      }
      QFEC_HIP(plan->cbook.ensure(book.size()));
      QFEC_HIP(hipMemcpy(plan->cbook.ptr, book.data(), book.size(), hipMemcpyHostToDevice));
    }
    a.compact_tables = true;
    a.codebook = plan->cbook.as<uint8_t>();
    a.meta = level_meta(plan->clayout, r);
  }
  if (row_start != nullptr) {
    // refused, one recover_runs launch, or the row prefix + the mask-addressed decode_fused
    const qfec::PackedForm packed = qfec::packed_form(a, form, qfec::test_knob(qfec::TestKnob::kPackedRuns, -1));
    if (packed == qfec::PackedForm::kRefused) {
      set_error("packed recover: no mask-addressed form for k=%u r=%u P=%u (use fec_recover_batch_rs_dev)", k, r, P);
      return FEC_ERR_RANGE;
    }
    if (packed == qfec::PackedForm::kRuns) {
      qfec::RunsLaunch ra{};
      ra.data = c.data;
      ra.parity = c.parity;
      ra.masks = d_masks;
      ra.groups = G;
      ra.k = k;
      ra.r = r;
      ra.P = P;
      ra.codebook = a.codebook;
      ra.meta = a.meta;
      ra.out = d_out;
      ra.row_start = row_start;
      ra.total = row_total;
      ra.status = d_status;
      QFEC_HIP(runs_workspace(ctx, s, G, &ra.workspace, &ra.epoch));
      QFEC_HIP(qfec::launch_recover_runs(ra, s));
      return FEC_OK;
    }
    a.rec_off = row_start;
    a.packed_rows = true;
    // the form exists: now the row starts (two small launches ahead of the recover; the block
    // sums use the stream's workspace, which this path does not otherwise take)
    void* ws = nullptr;
    QFEC_HIP(stream_workspace(ctx, s, qfec::rows_prefix_workspace_bytes(G), &ws));
    QFEC_HIP(qfec::launch_rows_prefix(d_masks, G, k, r, row_start, static_cast<uint32_t*>(ws), row_total, s));
  }
  if (!plan->dense && c.device_masks && ctx->plan_mode == FEC_PLAN_DEVICE) {
    // Records built on the device, in the caller stream's workspace, chunk after chunk ahead of
    // the form's kernels: nothing comes to the host and the call is asynchronous on s.
    qfec::PlanWorkspace w;
    uint8_t* ws = nullptr;
    rc = plan_workspace_locked(ctx, plan, s, G, k, r, false, false, &w, &ws, &a.plan);
    if (rc != FEC_OK) return rc;
    a.rec_off = reinterpret_cast<uint32_t*>(ws + w.rec_off);
    a.codebook = a.plan.arena;
    QFEC_HIP(qfec::launch_decode(a, s));
    return FEC_OK;
  }
  // Workspace: the caller's slot buffer (pipeline slots: private stream, calls serialised
  // by the context lock), else one private to this call.
  if (row_start == nullptr && form.rec_off) {
    if (rec) {
      QFEC_HIP(rec->ensure(G * sizeof(uint32_t)));
      a.rec_off = rec->as<uint32_t>();
    } else {
      void* ws = nullptr;
      QFEC_HIP(stream_workspace(ctx, s, G * sizeof(uint32_t), &ws));
      a.rec_off = static_cast<uint32_t*>(ws);
    }
  }
  std::vector<uint8_t> book, st;
  std::vector<uint32_t> ro;
  if (!plan->dense) {
    // Sparse plan: the masks come to the host (after the stream's earlier work), records
    // are built for the patterns present, and the call completes synchronously.
    std::vector<uint64_t> hm(G);
    QFEC_HIP(hipStreamSynchronize(s));
    QFEC_HIP(hipMemcpy(hm.data(), d_masks, G * 8, hipMemcpyDefault));
    if (!qfec::build_sparse_plan(k, r, plan->M, hm.data(), G, qfec::kRecNone, qfec::kRecBad, book, ro, st)) {
      set_error("decode: sparse plan failed for k=%u r=%u", k, r);
      return FEC_ERR_RANGE;
    }
    QFEC_HIP(plan->sparse_book.ensure(book.size() + 32));
    if (!book.empty())
      QFEC_HIP(hipMemcpyAsync(plan->sparse_book.ptr, book.data(), book.size(), hipMemcpyHostToDevice, s));
    QFEC_HIP(hipMemcpyAsync(a.rec_off, ro.data(), G * 4, hipMemcpyHostToDevice, s));
    if (d_status) QFEC_HIP(hipMemcpyAsync(d_status, st.data(), G, hipMemcpyDefault, s));
    a.codebook = plan->sparse_book.as<uint8_t>();
  }
  QFEC_HIP(qfec::launch_decode(a, s));
  // sparse: the records (and the host vectors above) are reused / freed after this call
  if (!plan->dense) QFEC_HIP(hipStreamSynchronize(s));
  return FEC_OK;
}

// A pipelined call that fails part-way returns only after its slots' streams have drained:
// earlier chunks' copies still read the caller's buffers and write its outputs.
struct PipeDrain {
  FECEncoderCtx* ctx;
  bool done = false;
  ~PipeDrain() {
    if (done) return;
    for (auto& p : ctx->pipe)
      if (p.s) (void)hipStreamSynchronize(p.s);
    (void)hipGetLastError();
  }
};

int ensure_pipe(FECEncoderCtx* ctx) {
  for (auto& p : ctx->pipe)
    if (!p.s) QFEC_HIP(hipStreamCreateWithFlags(&p.s, hipStreamNonBlocking));
  return FEC_OK;
}

int sync_slot(PipeSlot& p) {
  QFEC_HIP(hipStreamSynchronize(p.s));
  return FEC_OK;
}

// The chunk pipeline of the host-resident batches: N groups of in_g data bytes each in chunks of
// ~64 MB of data (fec_routes.hpp), chunk c on pipeline slot c % 3.  ensure(p, cg) grows slot p's
// buffers for chunks of cg groups; body(sl, first, n) queues the groups [first, first + n) on slot
// sl; retire(p) waits for slot p's chunk and finishes it: for every slot at the end of the call
// and, with retire_before_refill, before a slot takes its next chunk.
template <class Ensure, class Body, class Retire>
int run_pipeline(FECEncoderCtx* ctx, uint64_t N, uint64_t in_g, bool retire_before_refill, Ensure ensure, Body body,
                 Retire retire) {
  int rc = ensure_pipe(ctx);
  if (rc != FEC_OK) return rc;
  PipeDrain drain{ctx};
  const uint64_t cg = qfec::pipe_chunk_groups(pipe_chunk_bytes(), in_g, N);
  for (auto& p : ctx->pipe)
    if ((rc = ensure(p, cg)) != FEC_OK) return rc;
  uint64_t c = 0;
  for (uint64_t first = 0; first < N; first += cg, ++c) {
    PipeSlot& sl = ctx->pipe[c % kPipeSlots];
    if (retire_before_refill && (rc = retire(sl)) != FEC_OK) return rc;
    if ((rc = body(sl, first, N - first < cg ? N - first : cg)) != FEC_OK) return rc;
  }
  for (auto& p : ctx->pipe)
    if ((rc = retire(p)) != FEC_OK) return rc;
  drain.done = true;
  return FEC_OK;
}

// Host-resident batches: H2D -> kernel -> D2H per chunk.  Page-locked host buffers
// (fec_alloc_slab) make the copies asynchronous; pageable ones still work, with less overlap.
int encode_host_pipelined(FECEncoderCtx* ctx, const uint8_t* data, uint64_t G, uint32_t k, uint32_t r,
                          uint32_t P, uint8_t* parity_out) {
  const uint64_t in_g = uint64_t(k) * P, out_g = uint64_t(r) * P;
  return run_pipeline(
      ctx, G, in_g, false,
      [&](PipeSlot& p, uint64_t cg) {
        QFEC_HIP(p.in.ensure(cg * in_g));
        QFEC_HIP(p.par.ensure(cg * out_g));
        return FEC_OK;
      },
      [&](PipeSlot& sl, uint64_t g0, uint64_t n) {
        QFEC_HIP(hipMemcpyAsync(sl.in.ptr, data + g0 * in_g, n * in_g, hipMemcpyHostToDevice, sl.s));
        const int rc = encode_dev_locked(ctx, sl.in.as<uint8_t>(), nullptr, qfec::OffsetKind::kNone, n, k, r, P,
                                         sl.par.as<uint8_t>(), sl.s);
        if (rc != FEC_OK) return rc;
        QFEC_HIP(hipMemcpyAsync(parity_out + g0 * out_g, sl.par.ptr, n * out_g, hipMemcpyDeviceToHost, sl.s));
        return FEC_OK;
      },
      sync_slot);
}

int decode_host_pipelined(FECEncoderCtx* ctx, uint8_t* data, const uint8_t* parity, const uint64_t* masks,
                          uint64_t G, uint32_t k, uint32_t r, uint32_t P, uint8_t* status_out) {
  const uint64_t in_g = uint64_t(k) * P, par_g = uint64_t(r) * P;
  // Page-locked data: the kernel stores the rebuilt shards straight into host memory
  // (zero-copy PCIe writes of ~e*P bytes per group) instead of a D2H of the whole chunk.
  uint8_t* host_dev = nullptr;
  if (classify_ptr(data) == Mem::kPinned) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, data) == hipSuccess && attr.devicePointer)
      host_dev = static_cast<uint8_t*>(attr.devicePointer);
    else
      (void)hipGetLastError();
  }
  return run_pipeline(
      ctx, G, in_g, false,
      [&](PipeSlot& p, uint64_t cg) {
        QFEC_HIP(p.in.ensure(cg * in_g));
        QFEC_HIP(p.par.ensure(cg * par_g));
        QFEC_HIP(p.mask.ensure(cg * 8));
        QFEC_HIP(p.status.ensure(cg));
        return FEC_OK;
      },
      [&](PipeSlot& sl, uint64_t g0, uint64_t n) {
        QFEC_HIP(hipMemcpyAsync(sl.in.ptr, data + g0 * in_g, n * in_g, hipMemcpyHostToDevice, sl.s));
        QFEC_HIP(hipMemcpyAsync(sl.par.ptr, parity + g0 * par_g, n * par_g, hipMemcpyHostToDevice, sl.s));
        QFEC_HIP(hipMemcpyAsync(sl.mask.ptr, masks + g0, n * 8, hipMemcpyHostToDevice, sl.s));
        DecodeCall c;
        c.data = sl.in.as<uint8_t>(), c.parity = sl.par.as<uint8_t>(), c.masks = sl.mask.as<uint64_t>();
        c.shape = {n, k, r, P}, c.status = sl.status.as<uint8_t>(), c.stream = sl.s, c.rec = &sl.rec;
        c.out = host_dev ? host_dev + g0 * in_g : nullptr;
        const int rc = decode_dev_locked(ctx, c);
        if (rc != FEC_OK) return rc;
        if (!host_dev)
          QFEC_HIP(hipMemcpyAsync(data + g0 * in_g, sl.in.ptr, n * in_g, hipMemcpyDeviceToHost, sl.s));
        QFEC_HIP(hipMemcpyAsync(status_out + g0, sl.status.ptr, n, hipMemcpyDeviceToHost, sl.s));
        return FEC_OK;
      },
      sync_slot);
}

// Host-resident decode when few groups lost data shards (e.g. the satellite profile, iid
// loss p = 0.01: ~11% of k=10 r=3 groups): only those groups cross PCIe.  Per chunk, host
// threads gather the groups' data and parity into page-locked staging, the chunk goes
// H2D -> decode -> D2H on its pipeline slot, and the rebuilt packets are scattered back
// into `data`.  Slot c % 3's previous chunk is scattered before its staging is refilled,
// so the CPU gather of one chunk overlaps the copies and kernels of the two before it.
// `need` lists the groups with lost data that are recoverable (status 0); everything
// else needs no device work.
int decode_host_compacted(FECEncoderCtx* ctx, uint8_t* data, const uint8_t* parity, const uint64_t* masks,
                          const std::vector<uint64_t>& need, uint32_t k, uint32_t r, uint32_t P) {
  const uint64_t in_g = uint64_t(k) * P, par_g = uint64_t(r) * P;
  // Rebuilt packets of the slot's last chunk: D2H landed in h_in; copy the erased ones out.
  const auto scatter = [&](PipeSlot& sl) {
    if (sl.h_groups.empty()) return FEC_OK;
    QFEC_HIP(hipStreamSynchronize(sl.s));
    const uint8_t* src = sl.h_in.as<uint8_t>();
    const uint64_t* gl = sl.h_groups.data();
    parallel_for(sl.h_groups.size(), 512, [&](uint64_t b, uint64_t e) {
      for (uint64_t i = b; i < e; ++i) {
        const uint64_t g = gl[i];
        qfec::for_each_lost(masks[g], k, [&](uint32_t j) {
          std::memcpy(data + g * in_g + uint64_t(j) * P, src + i * in_g + uint64_t(j) * P, P);
        });
      }
    });
    sl.h_groups.clear();
    return FEC_OK;
  };
  return run_pipeline(
      ctx, need.size(), in_g, /*retire_before_refill=*/true,
      [&](PipeSlot& p, uint64_t cg) {
        QFEC_HIP(p.in.ensure(cg * in_g));
        QFEC_HIP(p.par.ensure(cg * par_g));
        QFEC_HIP(p.mask.ensure(cg * 8));
        QFEC_HIP(p.h_in.ensure(cg * in_g));
        QFEC_HIP(p.h_par.ensure(cg * par_g));
        QFEC_HIP(p.h_mask.ensure(cg * 8));
        p.h_groups.clear();
        return FEC_OK;
      },
      [&](PipeSlot& sl, uint64_t i0, uint64_t n) {
        const uint64_t* gl = need.data() + i0;
        uint8_t* hi = sl.h_in.as<uint8_t>();
        uint8_t* hp = sl.h_par.as<uint8_t>();
        uint64_t* hm = sl.h_mask.as<uint64_t>();
        parallel_for(n, 512, [&](uint64_t b, uint64_t e) {
          for (uint64_t i = b; i < e; ++i) {
            const uint64_t g = gl[i];
            std::memcpy(hi + i * in_g, data + g * in_g, in_g);
            std::memcpy(hp + i * par_g, parity + g * par_g, par_g);
            hm[i] = masks[g];
          }
        });
        sl.h_groups.assign(gl, gl + n);
        QFEC_HIP(hipMemcpyAsync(sl.in.ptr, hi, n * in_g, hipMemcpyHostToDevice, sl.s));
        QFEC_HIP(hipMemcpyAsync(sl.par.ptr, hp, n * par_g, hipMemcpyHostToDevice, sl.s));
        QFEC_HIP(hipMemcpyAsync(sl.mask.ptr, hm, n * 8, hipMemcpyHostToDevice, sl.s));
        DecodeCall c;
        c.data = sl.in.as<uint8_t>(), c.parity = sl.par.as<uint8_t>(), c.masks = sl.mask.as<uint64_t>();
        c.shape = {n, k, r, P}, c.stream = sl.s, c.rec = &sl.rec;
        const int rc = decode_dev_locked(ctx, c);
        if (rc != FEC_OK) return rc;
        QFEC_HIP(hipMemcpyAsync(hi, sl.in.ptr, n * in_g, hipMemcpyDeviceToHost, sl.s));
        return FEC_OK;
      },
      scatter);
}

// Zero-copy view of a host buffer for a kernel: its own device address when page-locked,
// else the staging buffer `stage` (grown to `bytes`, filled from `host` when `fill`).
// `*staged` says which.
int zc_view(HostBuf& stage, const void* host, Mem m, void* dev, uint64_t bytes, bool fill, uint8_t** out,
            bool* staged) {
  if (m == Mem::kPinned && dev) {
    *out = static_cast<uint8_t*>(dev);
    *staged = false;
    return FEC_OK;
  }
  QFEC_HIP(stage.ensure(bytes));
  if (fill) std::memcpy(stage.ptr, host, bytes);
  *out = stage.dev_as<uint8_t>();
  *staged = true;
  return FEC_OK;
}

// Small host-resident encode, zero-copy (fec_routes.hpp).  Caller holds ctx->mu.
int encode_host_zero_copy(FECEncoderCtx* ctx, const uint8_t* data, Mem dmem, void* ddev, uint64_t G, uint32_t k,
                          uint32_t r, uint32_t P, uint8_t* parity_out, Mem omem, void* odev) {
  const uint64_t in_bytes = G * k * uint64_t(P), out_bytes = G * r * uint64_t(P);
  uint8_t *src = nullptr, *dst = nullptr;
  bool in_staged = false, out_staged = false;
  int rc = zc_view(ctx->z_in, data, dmem, ddev, in_bytes, true, &src, &in_staged);
  if (rc == FEC_OK) rc = zc_view(ctx->z_out, parity_out, omem, odev, out_bytes, false, &dst, &out_staged);
  if (rc == FEC_OK) rc = encode_dev_locked(ctx, src, nullptr, qfec::OffsetKind::kNone, G, k, r, P, dst, ctx->stream);
  if (rc != FEC_OK) return rc;
  QFEC_HIP(wait_stream(ctx->stream));
  if (out_staged) std::memcpy(parity_out, ctx->z_out.ptr, out_bytes);
  return FEC_OK;
}

// Small host-resident decode, zero-copy: survivors are read and rebuilt shards written in
// place through PCIe.  Statuses come from the caller's host scan.  Caller holds ctx->mu.
int decode_host_zero_copy(FECEncoderCtx* ctx, uint8_t* data, Mem dmem, void* ddev, const uint8_t* parity, Mem pmem,
                          void* pdev, const uint64_t* masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                          double need_share) {
  const uint64_t in_g = uint64_t(k) * P;
  uint8_t *d = nullptr, *p = nullptr;
  bool d_staged = false, p_staged = false;
  int rc = zc_view(ctx->z_in, data, dmem, ddev, G * in_g, true, &d, &d_staged);
  if (rc == FEC_OK) rc = zc_view(ctx->z_out, parity, pmem, pdev, G * r * uint64_t(P), true, &p, &p_staged);
  if (rc != FEC_OK) return rc;
  QFEC_HIP(ctx->z_aux.ensure(G * 8));
  std::memcpy(ctx->z_aux.ptr, masks, G * 8);
  DecodeCall c;
  c.data = d, c.parity = p, c.masks = ctx->z_aux.dev_as<uint64_t>();
  c.shape = {G, k, r, P}, c.stream = ctx->stream, c.need_share = need_share;
  rc = decode_dev_locked(ctx, c);
  if (rc != FEC_OK) return rc;
  QFEC_HIP(wait_stream(ctx->stream));
  if (d_staged) {  // only erased data packets changed (unrecoverable groups: untouched bytes)
    const uint8_t* z = ctx->z_in.as<uint8_t>();
    for (uint64_t g = 0; g < G; ++g)
      qfec::for_each_lost(masks[g], k, [&](uint32_t j) {
        const uint64_t o = g * in_g + uint64_t(j) * P;
        std::memcpy(data + o, z + o, P);
      });
  }
  return FEC_OK;
}

// Process-wide context used by the context-free xor_packets_* entry points.
FECEncoderCtx* default_ctx() {
  static std::once_flag once;
  static FECEncoderCtx* ctx = nullptr;
  std::call_once(once, [] { ctx = make_ctx(0.10, 1024, -1); });
  return ctx;
}

void xor_packets_gpu(const uint8_t* packets[], size_t n, size_t packet_size, uint8_t* repair) {
  g_last_error.clear();  // void return: callers read fec_hip_last_error() to detect failure
  if (n == 0 || packet_size == 0) return;  // fec_xor_simd.cpp:417-419
  if (!packets || !repair) {
    set_error("xor_packets: NULL argument");
    return;
  }
  if (packet_size > 0xFFFFFFFFull || n > 0xFFFFFFFFull) {
    set_error("xor_packets: size out of range");
    return;
  }
  FECEncoderCtx* ctx = default_ctx();
  if (!ctx) return;
  CtxBound bound(ctx);  // a device that does not bind shows in the calls below
  const uint32_t P = static_cast<uint32_t>(packet_size);
  if ((n + 1) * uint64_t(packet_size) <= small_call_limits().staged) {
    // Host packets: gather them into page-locked staging and run zero-copy.
    bool host = classify_ptr(repair) != Mem::kDevice;
    for (size_t p = 0; p < n && host; ++p) host = classify_ptr(packets[p]) != Mem::kDevice;
    if (host) {
      if (ctx->z_in.ensure(n * packet_size) != hipSuccess || ctx->z_out.ensure(packet_size) != hipSuccess) {
        set_error("xor_packets: page-locked staging allocation failed");
        return;
      }
      for (size_t p = 0; p < n; ++p) std::memcpy(ctx->z_in.as<uint8_t>() + p * packet_size, packets[p], packet_size);
      if (encode_dev_locked(ctx, ctx->z_in.dev_as<uint8_t>(), nullptr, qfec::OffsetKind::kNone, 1,
                            static_cast<uint32_t>(n), 1, P, ctx->z_out.dev_as<uint8_t>(), ctx->stream) != FEC_OK)
        return;
      if (wait_stream(ctx->stream) != hipSuccess) {
        set_error("xor_packets: kernel failed");
        return;
      }
      std::memcpy(repair, ctx->z_out.ptr, packet_size);
      return;
    }
  }
  // Stage the packets contiguously (k = n, one group, r = 1).
  if (ctx->d_in.ensure(n * packet_size) != hipSuccess || ctx->d_out.ensure(packet_size) != hipSuccess) {
    set_error("xor_packets: device allocation failed");
    return;
  }
  for (size_t p = 0; p < n; ++p) {
    if (hipMemcpyAsync(ctx->d_in.as<uint8_t>() + p * packet_size, packets[p], packet_size,
                       hipMemcpyDefault, ctx->stream) != hipSuccess) {
      set_error("xor_packets: H2D copy failed");
      return;
    }
  }
  if (encode_dev_locked(ctx, ctx->d_in.as<uint8_t>(), nullptr, qfec::OffsetKind::kNone, 1,
                        static_cast<uint32_t>(n), 1, P, ctx->d_out.as<uint8_t>(),
                        ctx->stream) != FEC_OK)
    return;
  if (hipMemcpyAsync(repair, ctx->d_out.ptr, packet_size, hipMemcpyDefault, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("xor_packets: D2H copy failed");
  }
}

}  // namespace

// =====================================================================================
// Reference ABI (include/fec_xor_simd.h)
// =====================================================================================

QFEC_EXPORT FECEncoderCtx* fec_encoder_new(double redundancy, uint32_t max_groups) {
  return make_ctx(redundancy, max_groups, -1);
}

QFEC_EXPORT void fec_encoder_free(FECEncoderCtx* ctx) { delete ctx; }

QFEC_EXPORT void* fec_alloc_slab(size_t size) {
  const size_t aligned = (size + 63) & ~size_t(63);  // fec_xor_simd.cpp:471
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, aligned == 0 ? 64 : aligned, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("fec_alloc_slab(%zu): %s", size, hipGetErrorString(e));
    return nullptr;
  }
  pinned_register(p, aligned == 0 ? 64 : aligned);
  return p;
}

namespace {

// NUMA-placed slabs (fec_alloc_slab_numa): mmap'd, mbind'd, then registered with HIP.
// fec_free_slab looks pointers up here to undo exactly what was done.
struct NumaSlab {
  size_t len;
  bool registered;
};
std::mutex g_numa_mu;
std::map<void*, NumaSlab> g_numa_slabs;

}  // namespace

QFEC_EXPORT void* fec_alloc_slab_numa(size_t size, int numa_node) {
  if (numa_node < 0) return fec_alloc_slab(size);
  const size_t page = static_cast<size_t>(sysconf(_SC_PAGESIZE));
  const size_t len = ((size == 0 ? 1 : size) + page - 1) / page * page;
  void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (p == MAP_FAILED) {
    set_error("fec_alloc_slab_numa(%zu): mmap: %s", size, std::strerror(errno));
    return nullptr;
  }
  // Bind before the first touch so every page is allocated on the node (fec_xor_simd.cpp:
  // 497-502 binds with MPOL_MF_MOVE and ignores failure; so does this -- e.g. a node the
  // machine does not have leaves the default policy).  The range is page-aligned, which
  // mbind requires.
  constexpr int kMaxNodes = 1024;
  unsigned long mask[kMaxNodes / (8 * sizeof(unsigned long))] = {};
  if (numa_node < kMaxNodes) {
    mask[numa_node / (8 * sizeof(unsigned long))] |= 1ul << (numa_node % (8 * sizeof(unsigned long)));
    constexpr int kMpolBind = 2, kMpolMfMove = 1 << 1;
    (void)syscall(SYS_mbind, p, len, kMpolBind, mask, static_cast<unsigned long>(kMaxNodes + 1), kMpolMfMove);
  }
  // Page-lock for DMA / zero-copy kernel access; pinning faults the pages in under the
  // policy above.  Without a GPU the memory stays pageable (the reference's behaviour).
  bool registered = false;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0)
    registered = hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess;
  (void)hipGetLastError();
  if (registered) pinned_register(p, len);
  std::lock_guard<std::mutex> lk(g_numa_mu);
  g_numa_slabs[p] = NumaSlab{len, registered};
  return p;
}

QFEC_EXPORT void* fec_alloc_repair_buffer(size_t size) { return fec_alloc_slab(size); }

QFEC_EXPORT void fec_free_slab(void* ptr) {
  if (!ptr) return;
  pinned_unregister(ptr);
  {
    std::lock_guard<std::mutex> lk(g_numa_mu);
    auto it = g_numa_slabs.find(ptr);
    if (it != g_numa_slabs.end()) {
      if (it->second.registered) (void)hipHostUnregister(ptr);
      (void)munmap(ptr, it->second.len);
      g_numa_slabs.erase(it);
      return;
    }
  }
  (void)hipHostFree(ptr);
}

QFEC_EXPORT void fec_free_repair_buffer(void* ptr) { fec_free_slab(ptr); }

// What fec_coalesce.cpp borrows (fec_internal.hpp).
namespace qfec {

int encode_addr_batch(FECEncoderCtx* ctx, const uint64_t* d_addr, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                      uint8_t* d_parity, hipStream_t s) {
  CtxBound bound(ctx, "fec_encode_batch");
  if (bound.rc != FEC_OK) return bound.rc;
  return encode_dev_locked(ctx, nullptr, d_addr, OffsetKind::kAddr, G, k, r, P, d_parity, s);
}

void set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }

}  // namespace qfec

QFEC_EXPORT int fec_encode_batch(FECEncoderCtx* ctx, const uint8_t* slab, const uint32_t* offsets,
                                 uint32_t num_groups, uint32_t packet_size, uint8_t* repair_out) {
  return api_call(ctx, [&]() -> int {
    // fec_xor_simd.cpp:564-570, same order
    if (ctx == nullptr || slab == nullptr || offsets == nullptr || repair_out == nullptr) return -1;
    if (num_groups == 0 || packet_size == 0) return 0;
    // Small host-resident calls -- the reference's one group per call from each stream's own
    // context -- share launches with every other context's (fec_coalesce.cpp).
    int crc = 0;
    if (qfec::coalesce_legacy_encode(ctx->device, slab, offsets, num_groups, packet_size, repair_out, &crc, ctx->stream))
      return crc;
    constexpr uint32_t kPackets = 10;  // fec_xor_simd.cpp:580
    CtxBound bound(ctx, "fec_encode_batch");
    if (bound.rc != FEC_OK) return bound.rc;
    const uint64_t noff = uint64_t(num_groups) * kPackets;
    const uint64_t P = packet_size;
    void *slab_dev = nullptr, *out_dev = nullptr;
    const Mem slab_mem = classify_ptr(slab, &slab_dev);
    const Mem off_mem = classify_ptr(offsets);
    const Mem out_mem = classify_ptr(repair_out, &out_dev);
    hipStream_t s = ctx->stream;
    // A host slab: its offsets are read here (brought back when they are on the device) to size
    // the slab window.
    std::vector<uint32_t> host_off;
    const uint32_t* hoff = offsets;
    qfec::OffsetWindow<uint32_t> win{};
    if (slab_mem != Mem::kDevice) {
      if (off_mem == Mem::kDevice) {
        host_off.resize(noff);
        QFEC_HIP(hipMemcpy(host_off.data(), offsets, noff * 4, hipMemcpyDeviceToHost));
        hoff = host_off.data();
      }
      win = qfec::offset_window(hoff, noff, P);
    }
    const uint32_t lo = win.lo;
    const uint64_t span = win.span;
    const qfec::LegacyEncodeRoute route =
        qfec::legacy_encode_route(slab_mem, out_mem, (noff + num_groups) * P, span, small_call_limits());
    switch (route.route) {
      case qfec::EncodeRoute::kZeroCopy: {
        // offsets (rebased to the staged window unless the slab is page-locked) and the slab window
        // in page-locked memory, read by the kernel over PCIe
        QFEC_HIP(ctx->z_aux.ensure(noff * 4));
        uint32_t* zo = ctx->z_aux.as<uint32_t>();
        const uint8_t* zs = static_cast<const uint8_t*>(slab_dev);
        if (route.rebase) {
          QFEC_HIP(ctx->z_in.ensure(span));
          std::memcpy(ctx->z_in.ptr, slab + lo, span);
          qfec::rebase_offsets(hoff, noff, lo, zo);
          zs = ctx->z_in.dev_as<uint8_t>();
        } else {
          std::memcpy(zo, hoff, noff * 4);
        }
        uint8_t* zr = nullptr;
        bool out_staged = false;
        int rc = zc_view(ctx->z_out, repair_out, out_mem, out_dev, uint64_t(num_groups) * P, false, &zr, &out_staged);
        if (rc == FEC_OK)
          rc = encode_dev_locked(ctx, zs, ctx->z_aux.dev_as<uint32_t>(), qfec::OffsetKind::kU32, num_groups, kPackets,
                                 1, packet_size, zr, s);
        if (rc != FEC_OK) return rc;
        QFEC_HIP(wait_stream(s));
        if (out_staged) std::memcpy(repair_out, ctx->z_out.ptr, uint64_t(num_groups) * P);
        return 0;
      }
      default: {  // kStaged
        const uint8_t* d_slab = slab;
        const uint32_t* d_offsets = offsets;
        if (route.rebase) {
          // Copy the window [lo, hi + P) of the host slab; rebase offsets to it.
          std::vector<uint32_t> rebased(noff);
          qfec::rebase_offsets(hoff, noff, lo, rebased.data());
          QFEC_HIP(ctx->d_in.ensure(span));
          QFEC_HIP(ctx->d_off.ensure(noff * 4));
          QFEC_HIP(hipMemcpyAsync(ctx->d_in.ptr, slab + lo, span, hipMemcpyHostToDevice, s));
          QFEC_HIP(hipMemcpyAsync(ctx->d_off.ptr, rebased.data(), noff * 4, hipMemcpyHostToDevice, s));
          QFEC_HIP(hipStreamSynchronize(s));  // `rebased` dies at scope end
          d_slab = ctx->d_in.as<uint8_t>();
          d_offsets = ctx->d_off.as<uint32_t>();
        } else if (off_mem != Mem::kDevice) {
          QFEC_HIP(ctx->d_off.ensure(noff * 4));
          QFEC_HIP(hipMemcpyAsync(ctx->d_off.ptr, hoff, noff * 4, hipMemcpyHostToDevice, s));
          d_offsets = ctx->d_off.as<uint32_t>();
        }
        uint8_t* d_repair = repair_out;
        if (out_mem != Mem::kDevice) {
          QFEC_HIP(ctx->d_out.ensure(uint64_t(num_groups) * P));
          d_repair = ctx->d_out.as<uint8_t>();
        }
        const int rc = encode_dev_locked(ctx, d_slab, d_offsets, qfec::OffsetKind::kU32, num_groups, kPackets, 1,
                                         packet_size, d_repair, s);
        if (rc != FEC_OK) return rc;
        if (out_mem != Mem::kDevice)
          QFEC_HIP(hipMemcpyAsync(repair_out, d_repair, uint64_t(num_groups) * P, hipMemcpyDeviceToHost, s));
        QFEC_HIP(hipStreamSynchronize(s));
        return 0;
      }
    }
  });
}

QFEC_EXPORT xor_impl_fn fec_select_xor_impl(void) { return xor_packets_gpu; }

QFEC_EXPORT void xor_packets_scalar(const uint8_t* packets[], size_t n, size_t packet_size,
                                    uint8_t* repair) {
  xor_packets_gpu(packets, n, packet_size, repair);
}
QFEC_EXPORT void xor_packets_avx2(const uint8_t* packets[], size_t n, size_t packet_size,
                                  uint8_t* repair) {
  xor_packets_gpu(packets, n, packet_size, repair);
}
QFEC_EXPORT void xor_packets_avx512(const uint8_t* packets[], size_t n, size_t packet_size,
                                    uint8_t* repair) {
  xor_packets_gpu(packets, n, packet_size, repair);
}
QFEC_EXPORT void xor_packets_neon(const uint8_t* packets[], size_t n, size_t packet_size,
                                  uint8_t* repair) {
  xor_packets_gpu(packets, n, packet_size, repair);
}

// =====================================================================================
// Batch GF(2^8) API (include/fec_hip.h)
// =====================================================================================

QFEC_EXPORT int fec_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

QFEC_EXPORT const char* fec_hip_last_error(void) { return g_last_error.c_str(); }

QFEC_EXPORT size_t fec_ctx_last_error(FECEncoderCtx* ctx, char* buf, size_t buflen) {
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  if (buf && buflen > 0) {
    const size_t n = ctx->last_error.size() < buflen - 1 ? ctx->last_error.size() : buflen - 1;
    std::memcpy(buf, ctx->last_error.data(), n);
    buf[n] = '\0';
  }
  return ctx->last_error.size();
}

QFEC_EXPORT FECEncoderCtx* fec_encoder_new_device(double redundancy, uint32_t max_groups, int device) {
  if (device < 0) {
    set_error("fec_encoder_new_device: negative device");
    return nullptr;
  }
  return make_ctx(redundancy, max_groups, device);
}

QFEC_EXPORT int fec_encoder_device(const FECEncoderCtx* ctx) { return ctx ? ctx->device : -1; }

extern "C" const char qfec_src_hash[];  // src_hash.o, generated by src_hash.py at build time

QFEC_EXPORT const char* fec_hip_version(void) {
  static const std::string v = std::string("libfec_hip 0.2 gfx950 src=") + qfec_src_hash;
  return v.c_str();
}

QFEC_EXPORT int fec_parity_matrix(uint32_t k, uint32_t r, uint8_t* out) {
  if (!out) return FEC_ERR_NULL;
  std::vector<uint8_t> M;
  if (!qfec::parity_matrix(k, r, M)) return FEC_ERR_RANGE;
  std::memcpy(out, M.data(), M.size());
  return FEC_OK;
}

namespace {

int check_shape(uint64_t G, uint32_t k, uint32_t r, uint32_t P, bool decode) {
  if (k == 0 || r == 0 || k + r > (decode ? qfec::kMaxDecodeShards : 256u)) {
    set_error("unsupported k=%u r=%u", k, r);
    return FEC_ERR_RANGE;
  }
  if (P == 0 && G != 0) {
    set_error("packet_size must be > 0");
    return FEC_ERR_RANGE;
  }
  return FEC_OK;
}

// fec_encode_batch_rs with a buffer on the device or packets at offsets: whatever is on the host
// goes through the context's device buffers in one shot (a host slab: its window, offsets rebased).
int encode_staged(FECEncoderCtx* ctx, const uint8_t* data, Mem dmem, const uint64_t* offsets, uint64_t G, uint32_t k,
                  uint32_t r, uint32_t P, uint8_t* parity_out, Mem omem) {
  hipStream_t s = ctx->stream;
  const uint64_t nin = G * k;
  const uint64_t out_bytes = G * r * uint64_t(P);
  const uint8_t* d_data = data;
  const void* d_off = nullptr;
  qfec::OffsetKind ok = qfec::OffsetKind::kNone;
  std::vector<uint64_t> rebased;
  if (offsets) {
    ok = qfec::OffsetKind::kU64;
    const Mem offmem = classify_ptr(offsets);
    std::vector<uint64_t> host_off;
    const uint64_t* hoff = offsets;
    if (offmem == Mem::kDevice) {
      host_off.resize(nin);
      QFEC_HIP(hipMemcpy(host_off.data(), offsets, nin * 8, hipMemcpyDeviceToHost));
      hoff = host_off.data();
    }
    if (dmem == Mem::kDevice) {
      if (offmem != Mem::kDevice) {
        QFEC_HIP(ctx->d_off.ensure(nin * 8));
        QFEC_HIP(hipMemcpyAsync(ctx->d_off.ptr, hoff, nin * 8, hipMemcpyHostToDevice, s));
        QFEC_HIP(hipStreamSynchronize(s));
        d_off = ctx->d_off.ptr;
      } else {
        d_off = offsets;
      }
    } else {
      const auto [lo, hi, span] = qfec::offset_window(hoff, nin, P);
      rebased.resize(nin);
      qfec::rebase_offsets(hoff, nin, lo, rebased.data());
      QFEC_HIP(ctx->d_in.ensure(span));
      QFEC_HIP(ctx->d_off.ensure(nin * 8));
      QFEC_HIP(hipMemcpyAsync(ctx->d_in.ptr, data + lo, span, hipMemcpyHostToDevice, s));
      QFEC_HIP(hipMemcpyAsync(ctx->d_off.ptr, rebased.data(), nin * 8, hipMemcpyHostToDevice, s));
      d_data = ctx->d_in.as<uint8_t>();
      d_off = ctx->d_off.ptr;
    }
  } else {
    if (dmem != Mem::kDevice) {
      QFEC_HIP(ctx->d_in.ensure(nin * P));
      QFEC_HIP(hipMemcpyAsync(ctx->d_in.ptr, data, nin * P, hipMemcpyHostToDevice, s));
      d_data = ctx->d_in.as<uint8_t>();
    }
  }
  uint8_t* d_par = parity_out;
  if (omem != Mem::kDevice) {
    QFEC_HIP(ctx->d_out.ensure(out_bytes));
    d_par = ctx->d_out.as<uint8_t>();
  }
  const int rc = encode_dev_locked(ctx, d_data, d_off, ok, G, k, r, P, d_par, s);
  if (rc != FEC_OK) return rc;
  if (omem != Mem::kDevice)
    QFEC_HIP(hipMemcpyAsync(parity_out, d_par, out_bytes, hipMemcpyDeviceToHost, s));
  QFEC_HIP(hipStreamSynchronize(s));
  return FEC_OK;
}

// fec_decode_batch_rs with a buffer on the device: the others go through the context's device
// buffers in one shot, and the statuses come back from the kernel.
int decode_staged(FECEncoderCtx* ctx, uint8_t* data, const uint8_t* parity, const uint64_t* masks,
                  const qfec::DecodeMem& mem, uint64_t G, uint32_t k, uint32_t r, uint32_t P, uint8_t* status_out,
                  uint64_t* unrecoverable_out) {
  hipStream_t s = ctx->stream;
  const uint64_t data_bytes = G * k * uint64_t(P);
  const uint64_t par_bytes = G * r * uint64_t(P);
  uint8_t* d_data = data;
  const uint8_t* d_par = parity;
  const uint64_t* d_masks = masks;
  if (mem.data != Mem::kDevice) {
    QFEC_HIP(ctx->d_in.ensure(data_bytes));
    QFEC_HIP(hipMemcpyAsync(ctx->d_in.ptr, data, data_bytes, hipMemcpyHostToDevice, s));
    d_data = ctx->d_in.as<uint8_t>();
  }
  if (mem.parity != Mem::kDevice) {
    QFEC_HIP(ctx->d_out.ensure(par_bytes));
    QFEC_HIP(hipMemcpyAsync(ctx->d_out.ptr, parity, par_bytes, hipMemcpyHostToDevice, s));
    d_par = ctx->d_out.as<uint8_t>();
  }
  if (mem.masks != Mem::kDevice) {
    QFEC_HIP(ctx->d_mask.ensure(G * 8));
    QFEC_HIP(hipMemcpyAsync(ctx->d_mask.ptr, masks, G * 8, hipMemcpyHostToDevice, s));
    d_masks = ctx->d_mask.as<uint64_t>();
  }
  QFEC_HIP(ctx->d_status.ensure(G));
  DecodeCall c;
  c.data = d_data, c.parity = d_par, c.masks = d_masks;
  c.shape = {G, k, r, P}, c.status = ctx->d_status.as<uint8_t>(), c.stream = s;
  const int rc = decode_dev_locked(ctx, c);
  if (rc != FEC_OK) return rc;
  if (mem.data != Mem::kDevice)
    QFEC_HIP(hipMemcpyAsync(data, d_data, data_bytes, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> st(G);
  QFEC_HIP(hipMemcpyAsync(st.data(), ctx->d_status.ptr, G, hipMemcpyDeviceToHost, s));
  QFEC_HIP(hipStreamSynchronize(s));
  uint64_t bad = 0;
  for (uint64_t g = 0; g < G; ++g) bad += st[g] != 0;
  if (status_out) std::memcpy(status_out, st.data(), G);
  if (unrecoverable_out) *unrecoverable_out = bad;
  return FEC_OK;
}

}  // namespace

QFEC_EXPORT int fec_encode_batch_rs(FECEncoderCtx* ctx, const uint8_t* data, const uint64_t* offsets,
                                    uint64_t G, uint32_t k, uint32_t r, uint32_t P, uint8_t* parity_out) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !data || !parity_out) return FEC_ERR_NULL;
    const int rc = check_shape(G, k, r, P, false);
    if (rc != FEC_OK) return rc;
    if (G == 0) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    void *ddev = nullptr, *odev = nullptr;
    const Mem dmem = classify_ptr(data, &ddev);
    const Mem omem = classify_ptr(parity_out, &odev);
    switch (qfec::encode_route(dmem, omem, offsets != nullptr, G * (k + r) * uint64_t(P), small_call_limits())) {
      case qfec::EncodeRoute::kZeroCopy:
        return encode_host_zero_copy(ctx, data, dmem, ddev, G, k, r, P, parity_out, omem, odev);
      case qfec::EncodeRoute::kPipelined:
        return encode_host_pipelined(ctx, data, G, k, r, P, parity_out);
      case qfec::EncodeRoute::kStaged:
        return encode_staged(ctx, data, dmem, offsets, G, k, r, P, parity_out, omem);
    }
    return FEC_ERR_RANGE;  // not reached
  });
}

QFEC_EXPORT int fec_decode_batch_rs(FECEncoderCtx* ctx, uint8_t* data, const uint8_t* parity,
                                    const uint64_t* masks, uint64_t G, uint32_t k, uint32_t r,
                                    uint32_t P, uint8_t* status_out, uint64_t* unrecoverable_out) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !data || !parity || !masks) return FEC_ERR_NULL;
    int rc = check_shape(G, k, r, P, true);
    if (rc != FEC_OK) return rc;
    if (unrecoverable_out) *unrecoverable_out = 0;
    if (G == 0) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    void *ddev = nullptr, *pdev = nullptr;
    qfec::DecodeMem mem{classify_ptr(data, &ddev), classify_ptr(parity, &pdev), classify_ptr(masks), Mem::kHost};
    if (status_out && mem.host_resident()) mem.status = classify_ptr(status_out);  // else it decides nothing
    // Host-resident: the masks are read here, once -- every status, the unrecoverable count and
    // which groups need work: lost data shards, and no more than the surviving parity rows.
    std::vector<uint8_t> st_local;
    uint8_t* st = status_out;
    std::vector<uint64_t> need;
    uint64_t bad = 0;
    if (mem.host_resident()) {
      if (!st) {
        st_local.resize(G);
        st = st_local.data();
      }
      for (uint64_t g = 0; g < G; ++g) {
        const qfec::MaskLosses ml = qfec::mask_losses(masks[g], k, r);
        st[g] = ml.unrecoverable ? 1 : 0;
        bad += ml.unrecoverable;
        if (ml.lost > 0 && !ml.unrecoverable) need.push_back(g);
      }
    }
    switch (qfec::decode_route(mem, G * (k + r) * uint64_t(P), G, need.size(), small_call_limits())) {
      case qfec::DecodeRoute::kNothing:
        break;
      case qfec::DecodeRoute::kZeroCopy:
        rc = decode_host_zero_copy(ctx, data, mem.data, ddev, parity, mem.parity, pdev, masks, G, k, r, P,
                                   double(need.size()) / double(G));
        break;
      case qfec::DecodeRoute::kCompacted:
        rc = decode_host_compacted(ctx, data, parity, masks, need, k, r, P);
        break;
      case qfec::DecodeRoute::kPipelined:  // the kernel's statuses land over the scan's: the same rule
        rc = decode_host_pipelined(ctx, data, parity, masks, G, k, r, P, st);
        break;
      case qfec::DecodeRoute::kStaged:
        return decode_staged(ctx, data, parity, masks, mem, G, k, r, P, status_out, unrecoverable_out);
    }
    if (rc != FEC_OK) return rc;
    if (unrecoverable_out) *unrecoverable_out = bad;
    return FEC_OK;
  });
}

QFEC_EXPORT int fec_encode_batch_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, uint64_t G,
                                        uint32_t k, uint32_t r, uint32_t P, uint8_t* d_parity,
                                        void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity) return FEC_ERR_NULL;
    const int rc = check_shape(G, k, r, P, false);
    if (rc != FEC_OK) return rc;
    if (G == 0) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    return encode_dev_locked(ctx, d_data, nullptr, qfec::OffsetKind::kNone, G, k, r, P, d_parity,
                             pick_stream(ctx, stream));
  });
}

QFEC_EXPORT int fec_decode_batch_rs_dev(FECEncoderCtx* ctx, uint8_t* d_data, const uint8_t* d_parity,
                                        const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r,
                                        uint32_t P, uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity || !d_masks) return FEC_ERR_NULL;
    const int rc = check_shape(G, k, r, P, true);
    if (rc != FEC_OK) return rc;
    if (G == 0) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    DecodeCall c;
    c.data = d_data, c.parity = d_parity, c.masks = d_masks;
    c.shape = {G, k, r, P}, c.status = d_status, c.stream = pick_stream(ctx, stream);
    c.device_masks = true;
    return decode_dev_locked(ctx, c);
  });
}

QFEC_EXPORT int fec_recover_batch_rs_dev_packed(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                                const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r,
                                                uint32_t P, uint8_t* d_rebuilt, uint32_t* d_row_start,
                                                uint64_t* d_total, uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity || !d_masks || !d_rebuilt || !d_row_start) return FEC_ERR_NULL;
    const int rc = check_shape(G, k, r, P, true);
    if (rc != FEC_OK) return rc;
    if (G * r >= (1ull << 32)) {
      set_error("packed recover: %llu groups x %u rows exceed 32-bit row indices", static_cast<unsigned long long>(G), r);
      return FEC_ERR_RANGE;
    }
    if (G == 0 && !d_total) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    if (G == 0) {
      QFEC_HIP(hipMemsetAsync(d_total, 0, sizeof(uint64_t), pick_stream(ctx, stream)));
      return FEC_OK;
    }
    // decode_dev_locked checks the form first and only then launches the row prefix, so an
    // unsupported shape returns FEC_ERR_RANGE with d_row_start / d_total untouched
    DecodeCall c;
    c.data = const_cast<uint8_t*>(d_data);  // the kernels only read `data` when the output is compact
    c.parity = d_parity, c.masks = d_masks, c.out = d_rebuilt, c.compact_out = true;
    c.shape = {G, k, r, P}, c.status = d_status, c.stream = pick_stream(ctx, stream);
    c.row_start = d_row_start, c.row_total = d_total;
    return decode_dev_locked(ctx, c);
  });
}

QFEC_EXPORT int fec_recover_batch_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                         const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                                         uint8_t* d_rebuilt, uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity || !d_masks || !d_rebuilt) return FEC_ERR_NULL;
    const int rc = check_shape(G, k, r, P, true);
    if (rc != FEC_OK) return rc;
    if (G == 0) return FEC_OK;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    DecodeCall c;
    c.data = const_cast<uint8_t*>(d_data);  // the kernels only read `data` when the output is compact
    c.parity = d_parity, c.masks = d_masks, c.out = d_rebuilt, c.compact_out = true;
    c.shape = {G, k, r, P}, c.status = d_status, c.stream = pick_stream(ctx, stream);
    c.device_masks = true;
    return decode_dev_locked(ctx, c);
  });
}

// ---- wide calls: k + r <= 256, four mask words per group (fec_wide.hip) ----
namespace {

// A refusal of the wide calls with the text every one of them reports; FEC_OK when served.
int wide_refusal(const char* what, qfec::WideRefusal why, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  switch (why) {
    case qfec::WideRefusal::kServed:
      break;
    case qfec::WideRefusal::kShape:
      set_error("%s: unsupported k=%u r=%u (need k>0, r>0, k+r<=%u)", what, k, r, qfec::kWideMaxShards);
      return FEC_ERR_RANGE;
    case qfec::WideRefusal::kRows:
      set_error("%s: k=%u r=%u: min(k, r) exceeds %u rows per group", what, k, r, qfec::kWideMaxRows);
      return FEC_ERR_RANGE;
    case qfec::WideRefusal::kPacket:
      set_error("%s: packet_size %u is below %u bytes", what, P, qfec::kVecMinP);
      return FEC_ERR_RANGE;
    case qfec::WideRefusal::kNoGroups:
      set_error("%s: num_groups is 0", what);
      return FEC_ERR_RANGE;
    case qfec::WideRefusal::kGroups:
      set_error("%s: %llu groups exceed 32-bit group indices", what, static_cast<unsigned long long>(G));
      return FEC_ERR_RANGE;
  }
  return FEC_OK;
}
// What wide_served refuses: the rule of a context in FEC_WIDE_ROWS_CAPPED, the default.
int wide_refused(const char* what, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  return wide_refusal(what, qfec::wide_served(G, k, r, P), G, k, r, P);
}
// A call wide_refused turned away with *rc, its text set: whether the context's rows mode serves it
// all the same, on the deep path (fec_forms.hpp wide_route; *rc is then FEC_OK).  Still refused,
// *rc and the text are wide_route's reason: in FEC_WIDE_ROWS_CAPPED the ones wide_refused gave.
bool wide_deep_admitted(const char* what, FECEncoderCtx* ctx, uint64_t G, uint32_t k, uint32_t r, uint32_t P, int* rc) {
  int mode;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    mode = ctx->wide_rows_mode;
  }
  const qfec::WideRoute route = qfec::wide_route(mode, G, k, r, P);
  g_last_error.clear();
  *rc = wide_refusal(what, route.why, G, k, r, P);
  return route.path == qfec::WidePath::kDeep;
}

// The shape's r x k parity matrix on the context's device (ctx->wide_matrices: one copy per (k, r),
// uploaded at the shape's first wide call).  The context's lock is held.
int wide_matrix(const char* what, FECEncoderCtx* ctx, uint32_t k, uint32_t r, const uint8_t** out) {
  auto& matrix = ctx->wide_matrices[std::make_pair(k, r)];
  if (!matrix) {
    std::vector<uint8_t> M;
    if (!qfec::parity_matrix(k, r, M)) {
      ctx->wide_matrices.erase(std::make_pair(k, r));
      set_error("%s: no parity matrix for k=%u r=%u", what, k, r);
      return FEC_ERR_RANGE;
    }
    auto buf = std::make_unique<DevBuf>();
    QFEC_HIP(buf->ensure(M.size()));
    QFEC_HIP(hipMemcpy(buf->ptr, M.data(), M.size(), hipMemcpyHostToDevice));
    matrix = std::move(buf);
  }
  *out = matrix->as<uint8_t>();
  return FEC_OK;
}

// What both wide calls do after their own NULL checks.  Refused before any lock or device call:
// whatever fec_forms.hpp wide_served refuses.  Then, under the context's lock and on its device:
// the shape's parity matrix on the device (one copy per (k, r), uploaded at the shape's first
// call), the stream -- a caller's stream counts for fec_encoder_free's drain as in every _dev call,
// and so does the workspace -- and the caller stream's workspace: G record offsets, then the record
// arena (wide_workspace).  The records are always built on the device; fec_decode_plan_mode is not
// consulted.  A shape wide_served refuses for its rows alone is served on the deep path when the
// context is in FEC_WIDE_ROWS_ALL (wide_deep_admitted): the same steps with wide_deep_arena's slots
// and fec_wide_deep.hip's launch.
int wide_call(const char* what, FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
              const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P, uint8_t* d_out, bool slots,
              uint8_t* d_status, void* stream) {
  int rc = wide_refused(what, G, k, r, P);
  const bool deep = rc != FEC_OK && wide_deep_admitted(what, ctx, G, k, r, P, &rc);
  if (rc != FEC_OK) return rc;
  CtxBound bound(ctx, what);
  if (bound.rc != FEC_OK) return bound.rc;
  const uint8_t* matrix = nullptr;
  rc = wide_matrix(what, ctx, k, r, &matrix);
  if (rc != FEC_OK) return rc;
  const hipStream_t s = pick_stream(ctx, stream);
  const uint64_t budget = qfec::plan_arena_budget();
  const qfec::PlanArena arena = deep ? qfec::wide_deep_arena(k, r, G, budget) : qfec::wide_arena(k, r, G, budget);
  const qfec::PlanWorkspace w = qfec::wide_workspace(G, arena);
  void* ws = nullptr;
  QFEC_HIP(stream_workspace(ctx, s, w.bytes, &ws));
  qfec::WideLaunch a{};
  a.data = d_data;
  a.parity = d_parity;
  a.out = d_out;
  a.slots = slots;
  a.masks = d_masks;
  a.rec_off = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws) + w.rec_off);
  a.status = d_status;
  a.groups = G;
  a.k = k, a.r = r, a.P = P;
  a.plan.arena = static_cast<uint8_t*>(ws) + w.arena;
  a.plan.stride = arena.stride;
  a.plan.per_chunk = arena.per_chunk;
  a.plan.matrix = matrix;
  QFEC_HIP(deep ? qfec::launch_decode_wide_deep(a, s) : qfec::launch_decode_wide(a, s));
  return FEC_OK;
}

}  // namespace

QFEC_EXPORT int fec_decode_wide_rs_dev(FECEncoderCtx* ctx, uint8_t* d_data, const uint8_t* d_parity,
                                       const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                                       uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity || !d_masks) {
      set_error("fec_decode_wide_rs_dev: %s is NULL", !ctx ? "the context" : !d_data ? "d_data" : !d_parity ? "d_parity" : "d_erasure_masks");
      return FEC_ERR_NULL;
    }
    return wide_call("fec_decode_wide_rs_dev", ctx, d_data, d_parity, d_masks, G, k, r, P, d_data, false, d_status, stream);
  });
}

QFEC_EXPORT int fec_recover_wide_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                        const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                                        uint8_t* d_rebuilt, uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_data || !d_parity || !d_masks || !d_rebuilt) {
      set_error("fec_recover_wide_rs_dev: %s is NULL",
                !ctx ? "the context" : !d_data ? "d_data" : !d_parity ? "d_parity" : !d_masks ? "d_erasure_masks" : "d_rebuilt");
      return FEC_ERR_NULL;
    }
    return wide_call("fec_recover_wide_rs_dev", ctx, d_data, d_parity, d_masks, G, k, r, P, d_rebuilt, true, d_status, stream);
  });
}

// ---- the wide recover from an address table into a table of destinations (fec_wide_table.hip) ----
// fec_recover_scatter_rs_dev for a wide shape: refused as the wide calls refuse, before any lock or
// device call; then the matrix, the stream and the caller stream's workspace (wide_table_workspace:
// record offsets, the masks when the caller gives no d_masks_out, the symbol lengths when there is a
// length table and the caller asks for none, the record arena).  Records on the device always.
QFEC_EXPORT int fec_recover_scatter_wide_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                                                const uint32_t* d_shard_lens, const uint64_t* d_dest_addrs, uint64_t G,
                                                uint32_t k, uint32_t r, uint32_t P, uint8_t* d_status,
                                                uint64_t* d_masks_out, uint32_t* d_symbol_len_out, void* stream) {
  return api_call(ctx, [&]() -> int {
    const char* what = "fec_recover_scatter_wide_rs_dev";
    if (!ctx || !d_shard_addrs || !d_dest_addrs) {
      set_error("%s: %s is NULL", what, !ctx             ? "the context"
                                        : !d_shard_addrs ? "d_shard_addrs"
                                                         : "d_dest_addrs (the destination table)");
      return FEC_ERR_NULL;
    }
    int rc = wide_refused(what, G, k, r, P);
    const bool deep = rc != FEC_OK && wide_deep_admitted(what, ctx, G, k, r, P, &rc);
    if (rc != FEC_OK) return rc;
    CtxBound bound(ctx, what);
    if (bound.rc != FEC_OK) return bound.rc;
    const uint8_t* matrix = nullptr;
    rc = wide_matrix(what, ctx, k, r, &matrix);
    if (rc != FEC_OK) return rc;
    const hipStream_t s = pick_stream(ctx, stream);
    const bool own_masks = d_masks_out == nullptr;
    const bool own_symlen = d_shard_lens != nullptr && d_symbol_len_out == nullptr;
    const uint64_t budget = qfec::plan_arena_budget();
    const qfec::PlanArena arena = deep ? qfec::wide_deep_arena(k, r, G, budget) : qfec::wide_arena(k, r, G, budget);
    const qfec::PlanWorkspace w = qfec::wide_table_workspace(G, own_masks, own_symlen, arena);
    void* ws = nullptr;
    QFEC_HIP(stream_workspace(ctx, s, w.bytes, &ws));
    uint8_t* base = static_cast<uint8_t*>(ws);
    qfec::WideTableLaunch a{};
    a.addrs = d_shard_addrs;
    a.lens = d_shard_lens;
    a.dests = d_dest_addrs;
    a.groups = G;
    a.k = k, a.r = r, a.P = P;
    a.status = d_status;
    a.masks = own_masks ? reinterpret_cast<uint64_t*>(base + w.masks) : d_masks_out;
    a.symlen = own_symlen ? reinterpret_cast<uint32_t*>(base + w.symlen) : d_symbol_len_out;
    a.rec_off = reinterpret_cast<uint32_t*>(base + w.rec_off);
    a.plan.arena = base + w.arena;
    a.plan.stride = arena.stride;
    a.plan.per_chunk = arena.per_chunk;
    a.plan.matrix = matrix;
    QFEC_HIP(deep ? qfec::launch_recover_scatter_wide_deep(a, s) : qfec::launch_recover_scatter_wide(a, s));
    return FEC_OK;
  });
}

// ---- packed recover for every shape (fec_packed.hip) ----
namespace {

// A refusal of the two packed calls with its text; FEC_OK when served.  The wide call's texts are
// the wide calls' (wide_refusal).
int packed_refusal(const char* what, bool wide, qfec::PackedRefusal why, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  using R = qfec::PackedRefusal;
  switch (why) {
    case R::kServed:
      return FEC_OK;
    case R::kShape:
      if (wide) return wide_refusal(what, qfec::WideRefusal::kShape, G, k, r, P);
      set_error("%s: unsupported k=%u r=%u (need k>0, r>0, k+r<=%u)", what, k, r, qfec::kPackedMaxShards);
      return FEC_ERR_RANGE;
    case R::kRows:
      return wide_refusal(what, qfec::WideRefusal::kRows, G, k, r, P);
    case R::kPacket:
      return wide_refusal(what, qfec::WideRefusal::kPacket, G, k, r, P);
    case R::kNoGroups:
      return wide_refusal(what, qfec::WideRefusal::kNoGroups, G, k, r, P);
    case R::kGroups:
      return wide_refusal(what, qfec::WideRefusal::kGroups, G, k, r, P);
    case R::kRowIndex:
      set_error("%s: %llu groups x %u rows exceed 32-bit row indices", what, static_cast<unsigned long long>(G), k < r ? k : r);
      return FEC_ERR_RANGE;
    case R::kNoCodebook:  // the address-table recovers' text: this call never reads masks back either
      set_error("%s: the codebook of k=%u r=%u exceeds the %llu-byte cap (sparse-plan shape: use "
                "fec_recover_batch_rs_dev, or fec_decode_plan_mode(ctx, FEC_PLAN_DEVICE))", what, k, r,
                static_cast<unsigned long long>(kCodebookCap));
      return FEC_ERR_RANGE;
  }
  return FEC_ERR_RANGE;
}

// The context's modes as packed_route's bits.
int packed_mode_bits(FECEncoderCtx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  return (ctx->plan_mode == FEC_PLAN_DEVICE ? qfec::kPackedPlanDevice : 0) |
         (ctx->wide_rows_mode == FEC_WIDE_ROWS_ALL ? qfec::kPackedRowsAll : 0);
}

struct PackedCall {
  const uint8_t *data, *parity;
  const uint64_t* masks;
  uint64_t G;
  uint32_t k, r, P;
  uint8_t* out;
  uint32_t* row_start;
  uint64_t* total;
  uint8_t* status;
  void* stream;
};

// A packed call on one of the new consumers (route.path kCodebook, kDevicePlan, kWide or kDeep),
// under the context's lock and on its device: the records' source, the stream, and ONE request to
// the caller stream's workspace for everything the call keeps there (packed_workspace: block sums,
// record offsets, the record arena).
int packed_call_locked(const char* what, FECEncoderCtx* ctx, const PackedCall& c, const qfec::PackedRoute& route) {
  const uint64_t G = c.G;
  const uint32_t k = c.k, r = c.r, P = c.P;
  CtxBound bound(ctx, what);
  if (bound.rc != FEC_OK) return bound.rc;
  qfec::PackedLaunch a{};
  a.path = route.path;
  int rc = FEC_OK;
  if (route.path == qfec::PackedPath::kCodebook || route.path == qfec::PackedPath::kDevicePlan) {
    DecodePlan* plan = nullptr;
    if ((rc = get_decode_plan(ctx, k, r, &plan)) != FEC_OK) return rc;
    a.binom = ctx->d_binom.as<uint64_t>();
    if (route.path == qfec::PackedPath::kCodebook) {
      a.codebook = plan->codebook.as<uint8_t>();
      a.meta = level_meta(plan->layout, r);
    } else if ((rc = plan_matrix(plan, &a.plan.matrix)) != FEC_OK) {
      return rc;
    }
  } else if ((rc = wide_matrix(what, ctx, k, r, &a.plan.matrix)) != FEC_OK) {
    return rc;
  }
  const hipStream_t s = pick_stream(ctx, c.stream);
  const qfec::PlanArena arena = qfec::packed_arena(route.path, k, r, G, qfec::plan_arena_budget());
  const qfec::PackedWorkspace w = qfec::packed_workspace(G, arena);
  void* ws = nullptr;
  QFEC_HIP(stream_workspace(ctx, s, w.bytes, &ws));
  uint8_t* base = static_cast<uint8_t*>(ws);
  a.data = c.data, a.parity = c.parity, a.masks = c.masks;
  a.groups = G, a.k = k, a.r = r, a.P = P;
  a.out = c.out, a.row_start = c.row_start, a.total = c.total, a.status = c.status;
  a.block_sums = reinterpret_cast<uint32_t*>(base + w.block_sums);
  a.rec_off = reinterpret_cast<uint32_t*>(base + w.rec_off);
  if (arena.bytes != 0) {
    a.plan.arena = base + w.arena;
    a.plan.stride = arena.stride;
    a.plan.per_chunk = arena.per_chunk;
  }
  QFEC_HIP(qfec::launch_recover_packed(a, s));
  return FEC_OK;
}

// The NULL checks of both packed calls; the message names the argument.
int packed_nulls(const char* what, FECEncoderCtx* ctx, const PackedCall& c, const char* masks_name) {
  const char* name = !ctx ? "the context" : !c.data ? "d_data" : !c.parity ? "d_parity" : !c.masks ? masks_name
                     : !c.out ? "d_rebuilt" : !c.row_start ? "d_row_start" : nullptr;
  if (name == nullptr) return FEC_OK;
  set_error("%s: %s is NULL", what, name);
  return FEC_ERR_NULL;
}

}  // namespace

QFEC_EXPORT int fec_recover_packed_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                          const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                                          uint8_t* d_rebuilt, uint32_t* d_row_start, uint64_t* d_total, uint8_t* d_status,
                                          void* stream) {
  return api_call(ctx, [&]() -> int {
    const char* what = "fec_recover_packed_rs_dev";
    const PackedCall c{d_data, d_parity, d_masks, G, k, r, P, d_rebuilt, d_row_start, d_total, d_status, stream};
    int rc = packed_nulls(what, ctx, c, "d_masks");
    if (rc != FEC_OK) return rc;
    qfec::CodebookLayout layout;
    const int bits = packed_mode_bits(ctx) | (qfec::codebook_layout(k, r, kCodebookCap, layout) ? qfec::kPackedDense : 0);
    const qfec::PackedRoute route = qfec::packed_route(bits, G, k, r, P);
    if ((rc = packed_refusal(what, false, route.why, G, k, r, P)) != FEC_OK) return rc;
    if (route.path == qfec::PackedPath::kEmpty) {
      if (!d_total) return FEC_OK;
      CtxBound bound(ctx, what);
      if (bound.rc != FEC_OK) return bound.rc;
      QFEC_HIP(hipMemsetAsync(d_total, 0, sizeof(uint64_t), pick_stream(ctx, stream)));
      return FEC_OK;
    }
    // what the old call serves is the old call's, byte for byte: its forms, its workspace, its errors
    if (route.path == qfec::PackedPath::kDelegate)
      return fec_recover_batch_rs_dev_packed(ctx, d_data, d_parity, d_masks, G, k, r, P, d_rebuilt, d_row_start, d_total,
                                             d_status, stream);
    return packed_call_locked(what, ctx, c, route);
  });
}

QFEC_EXPORT int fec_recover_packed_wide_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                               const uint64_t* d_masks, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                                               uint8_t* d_rebuilt, uint32_t* d_row_start, uint64_t* d_total,
                                               uint8_t* d_status, void* stream) {
  return api_call(ctx, [&]() -> int {
    const char* what = "fec_recover_packed_wide_rs_dev";
    const PackedCall c{d_data, d_parity, d_masks, G, k, r, P, d_rebuilt, d_row_start, d_total, d_status, stream};
    int rc = packed_nulls(what, ctx, c, "d_erasure_masks");
    if (rc != FEC_OK) return rc;
    const qfec::PackedRoute route = qfec::packed_wide_route(packed_mode_bits(ctx), G, k, r, P);
    if ((rc = packed_refusal(what, true, route.why, G, k, r, P)) != FEC_OK) return rc;
    return packed_call_locked(what, ctx, c, route);
  });
}

// ---- the wide encode from an address table into a table of destinations (fec_wide_encode.hip) ----
namespace {

// What wide_encode_served refuses, with the text the call reports; FEC_OK when served.  No rows
// cap: an encode builds no record.
int wide_encode_refused(const char* what, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  switch (qfec::wide_encode_served(G, k, r, P)) {
    case qfec::WideEncodeRefusal::kServed:
      break;
    case qfec::WideEncodeRefusal::kShape:
      set_error("%s: unsupported k=%u r=%u (need k>0, r>0, k+r<=%u)", what, k, r, qfec::kWideMaxShards);
      return FEC_ERR_RANGE;
    case qfec::WideEncodeRefusal::kPacket:
      set_error("%s: packet_size %u is below %u bytes", what, P, qfec::kVecMinP);
      return FEC_ERR_RANGE;
    case qfec::WideEncodeRefusal::kNoGroups:
      set_error("%s: num_groups is 0", what);
      return FEC_ERR_RANGE;
    case qfec::WideEncodeRefusal::kGroups:
      set_error("%s: %llu groups exceed 32-bit group indices", what, static_cast<unsigned long long>(G));
      return FEC_ERR_RANGE;
  }
  return FEC_OK;
}

// The shape's r x k coefficient table on the context's device, row 0 (the ones) as entries like
// any other row: encode_scatter_wide reads row m0 + m at tabs[(m0 + m) * k + j], so get_encode_plan's
// (r - 1) x k table, which leaves the XOR row out, does not serve it.  One copy per (k, r)
// (ctx->wide_enc_tables), uploaded at the shape's first call; r == 1 needs none (the XOR path).
// The context's lock is held.
int wide_encode_tables(const char* what, FECEncoderCtx* ctx, uint32_t k, uint32_t r, const void** out) {
  *out = nullptr;
  if (r == 1) return FEC_OK;
  auto& tables = ctx->wide_enc_tables[std::make_pair(k, r)];
  if (!tables) {
    std::vector<uint8_t> M;
    if (!qfec::parity_matrix(k, r, M)) {
      ctx->wide_enc_tables.erase(std::make_pair(k, r));
      set_error("%s: no parity matrix for k=%u r=%u", what, k, r);
      return FEC_ERR_RANGE;
    }
    std::vector<qfec::CoefEntry> tab(size_t(r) * k);
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = qfec::make_entry(M[i]);
    auto buf = std::make_unique<DevBuf>();
    QFEC_HIP(buf->ensure(tab.size() * sizeof(qfec::CoefEntry)));
    QFEC_HIP(hipMemcpy(buf->ptr, tab.data(), tab.size() * sizeof(qfec::CoefEntry), hipMemcpyHostToDevice));
    tables = std::move(buf);
  }
  *out = tables->ptr;
  return FEC_OK;
}

}  // namespace

// fec_encode_scatter_rs_dev for a wide shape: refused before any lock or device call; then the
// shape's coefficient table and the stream.  No classify, no record, no workspace.
QFEC_EXPORT int fec_encode_scatter_wide_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                                               const uint32_t* d_packet_lens, const uint64_t* d_dest_addrs, uint64_t G,
                                               uint32_t k, uint32_t r, uint32_t P, uint32_t* d_symbol_len_out,
                                               void* stream) {
  return api_call(ctx, [&]() -> int {
    const char* what = "fec_encode_scatter_wide_rs_dev";
    if (!ctx || !d_packet_addrs || !d_dest_addrs) {
      set_error("%s: %s is NULL", what, !ctx              ? "the context"
                                        : !d_packet_addrs ? "d_packet_addrs"
                                                          : "d_dest_addrs (the destination table)");
      return FEC_ERR_NULL;
    }
    int rc = wide_encode_refused(what, G, k, r, P);
    if (rc != FEC_OK) return rc;
    CtxBound bound(ctx, what);
    if (bound.rc != FEC_OK) return bound.rc;
    const void* tables = nullptr;
    rc = wide_encode_tables(what, ctx, k, r, &tables);
    if (rc != FEC_OK) return rc;
    const hipStream_t s = pick_stream(ctx, stream);
    // addrs, lens, dests, groups, k, r, P, symlen_out, tables
    const qfec::WideEncodeLaunch a{d_packet_addrs, d_packet_lens, d_dest_addrs, G, k, r, P, d_symbol_len_out, tables};
    QFEC_HIP(qfec::launch_encode_scatter_wide(a, s));
    return FEC_OK;
  });
}

// ---- address-table calls: shards / packets wherever they are in device memory ----
namespace {

// What both gather calls refuse before anything is launched or written; `what` names the call.
int check_gather_shape(const char* what, uint64_t G, uint32_t k, uint32_t r, uint32_t P) {
  if (k == 0 || r == 0) {
    set_error("%s: unsupported k=%u r=%u (need k>0, r>0)", what, k, r);
    return FEC_ERR_RANGE;
  }
  if (static_cast<uint64_t>(k) + r > qfec::kMaxDecodeShards) {
    set_error("%s: k=%u r=%u: k + r exceeds %u shards per group", what, k, r, qfec::kMaxDecodeShards);
    return FEC_ERR_RANGE;
  }
  if (P < qfec::kVecMinP) {
    set_error("%s: packet_size %u is below %u bytes", what, P, qfec::kVecMinP);
    return FEC_ERR_RANGE;
  }
  if (G == 0) {
    set_error("%s: num_groups is 0", what);
    return FEC_ERR_RANGE;
  }
  if (G >= (1ull << 32)) {
    set_error("%s: %llu groups exceed 32-bit group indices", what, static_cast<unsigned long long>(G));
    return FEC_ERR_RANGE;
  }
  return FEC_OK;
}

// The record-offset workspace step of the gather recovers, as a failure of it is reported.
constexpr const char* kRecOffWorkspaceCall = "stream_workspace(ctx, s, G * sizeof(uint32_t), &ws)";

// What the three table recovers do between their own NULL checks and their launch.  Refused
// before any lock or device call: the shape.  Refused under the context's lock, before a plan and
// its codebook are built: a codebook past the cap while the context is in FEC_PLAN_CODEBOOK (the
// sparse plan reads masks back on the host).  Then, on the context's device: the decode plan, the
// stream, the launch fields every table recover sets, and `ws_words` uint32_t per group of the
// caller stream's workspace (shared in stream order with the other decodes), the first G of them
// the record offsets, the second G (ws_words = 2: the scatter's own symbol lengths) a.symlen;
// `ws_call` is the text a failure of that step reports (each call's message as it was: QFEC_HIP
// reports the failing expression, and the calls wrote this one differently).  In FEC_PLAN_DEVICE a
// shape past the cap takes plan_workspace's layout instead -- record offsets, the masks when the
// caller gives no d_masks_out, the symbol lengths, the record arena -- and a.plan describes the
// arena.  launch(a, s) adds the call's own fields and launches, the lock still held.
template <typename F>
int table_recover_locked(const char* what, FECEncoderCtx* ctx, const uint64_t* d_shard_addrs, uint64_t G, uint32_t k,
                         uint32_t r, uint32_t P, uint8_t* d_status, uint64_t* d_masks_out, void* stream,
                         uint32_t ws_words, const char* ws_call, F launch) {
  int rc = check_gather_shape(what, G, k, r, P);
  if (rc != FEC_OK) return rc;
  qfec::CodebookLayout layout;
  const bool dense = qfec::codebook_layout(k, r, kCodebookCap, layout);
  CtxBound bound(ctx);
  if (!dense && ctx->plan_mode != FEC_PLAN_DEVICE) {
    set_error("%s: the codebook of k=%u r=%u exceeds the %llu-byte cap (sparse-plan shape: use "
              "fec_recover_batch_rs_dev, or fec_decode_plan_mode(ctx, FEC_PLAN_DEVICE))", what, k, r,
              static_cast<unsigned long long>(kCodebookCap));
    return FEC_ERR_RANGE;
  }
  if (bound.rc != FEC_OK) return bound.rc;
  DecodePlan* plan = nullptr;
  rc = get_decode_plan(ctx, k, r, &plan);
  if (rc != FEC_OK) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  qfec::TableRecoverLaunch a{};
  a.addrs = d_shard_addrs;
  a.groups = G;
  a.k = k;
  a.r = r;
  a.P = P;
  a.status = d_status;
  a.masks_out = d_masks_out;
  a.codebook = plan->codebook.as<uint8_t>();
  a.binom = ctx->d_binom.as<uint64_t>();
  a.meta = level_meta(plan->layout, r);
  if (!plan->dense) {
    qfec::PlanWorkspace w;
    uint8_t* pws = nullptr;
    rc = plan_workspace_locked(ctx, plan, s, G, k, r, d_masks_out == nullptr, ws_words == 2, &w, &pws, &a.plan);
    if (rc != FEC_OK) return rc;
    a.rec_off = reinterpret_cast<uint32_t*>(pws + w.rec_off);
    if (d_masks_out == nullptr) a.masks_out = reinterpret_cast<uint64_t*>(pws + w.masks);
    if (ws_words == 2) a.symlen = reinterpret_cast<uint32_t*>(pws + w.symlen);
    a.codebook = a.plan.arena;
    return launch(a, s);
  }
  void* ws = nullptr;
  const hipError_t we = stream_workspace(ctx, s, ws_words * G * sizeof(uint32_t), &ws);
  if (we != hipSuccess) return hip_fail(we, ws_call);
  a.rec_off = static_cast<uint32_t*>(ws);
  if (ws_words == 2) a.symlen = a.rec_off + G;
  return launch(a, s);
}

// What the three table encodes do between their own NULL checks and their launch: the shape,
// refused before any lock or device call; then, under the context's lock and on its device, the
// encode plan's coefficient tables and the stream.  launch(tables, s) fills the call's fields and
// launches, the lock still held.
template <typename F>
int table_encode_locked(const char* what, FECEncoderCtx* ctx, uint64_t G, uint32_t k, uint32_t r, uint32_t P,
                        void* stream, F launch) {
  int rc = check_gather_shape(what, G, k, r, P);
  if (rc != FEC_OK) return rc;
  CtxBound bound(ctx);
  if (bound.rc != FEC_OK) return bound.rc;
  const void* tables = nullptr;
  rc = get_encode_plan(ctx, k, r, &tables);
  if (rc != FEC_OK) return rc;
  return launch(tables, pick_stream(ctx, stream));
}

// The result of a table encode's launch; `call` is the text a failure reports, as `ws_call` above
// (QFEC_HIP reports the failing expression, and these calls' messages name the stream unpicked).
int table_encode_done(hipError_t e, const char* call) { return e == hipSuccess ? FEC_OK : hip_fail(e, call); }

}  // namespace

QFEC_EXPORT int fec_recover_gather_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs, uint64_t G, uint32_t k,
                                          uint32_t r, uint32_t P, uint8_t* d_rebuilt, uint8_t* d_status,
                                          uint64_t* d_masks_out, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_shard_addrs || !d_rebuilt) {
      set_error("gather recover: %s is NULL", !ctx ? "the context" : !d_shard_addrs ? "d_shard_addrs" : "d_rebuilt");
      return FEC_ERR_NULL;
    }
    return table_recover_locked("gather recover", ctx, d_shard_addrs, G, k, r, P, d_status, d_masks_out, stream, 1,
                                kRecOffWorkspaceCall, [&](qfec::TableRecoverLaunch& a, hipStream_t s) {
                                  a.out = d_rebuilt;
                                  QFEC_HIP(qfec::launch_recover_gather(a, s));
                                  return FEC_OK;
                                });
  });
}

QFEC_EXPORT int fec_encode_gather_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs, uint64_t G, uint32_t k,
                                         uint32_t r, uint32_t P, uint8_t* d_parity, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_packet_addrs || !d_parity) {
      set_error("gather encode: %s is NULL", !ctx ? "the context" : !d_packet_addrs ? "d_packet_addrs" : "d_parity");
      return FEC_ERR_NULL;
    }
    // launch_encode with absolute addresses: encode_dev_locked takes the plan's tables itself
    return table_encode_locked("gather encode", ctx, G, k, r, P, stream, [&](const void*, hipStream_t s) {
      return encode_dev_locked(ctx, nullptr, d_packet_addrs, qfec::OffsetKind::kAddr, G, k, r, P, d_parity, s);
    });
  });
}

// ---- the same with a length per table entry (fec_gather_var.hip) ----
QFEC_EXPORT int fec_recover_gather_var_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                                              const uint32_t* d_shard_lens, uint64_t G, uint32_t k, uint32_t r,
                                              uint32_t P, uint8_t* d_rebuilt, uint8_t* d_status,
                                              uint64_t* d_masks_out, uint32_t* d_symbol_len_out, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_shard_addrs || !d_shard_lens || !d_rebuilt) {
      set_error("variable-length gather recover: %s is NULL", !ctx             ? "the context"
                                                              : !d_shard_addrs ? "d_shard_addrs"
                                                              : !d_shard_lens  ? "d_shard_lens (the length table)"
                                                                               : "d_rebuilt");
      return FEC_ERR_NULL;
    }
    return table_recover_locked("variable-length gather recover", ctx, d_shard_addrs, G, k, r, P, d_status, d_masks_out,
                                stream, 1, kRecOffWorkspaceCall, [&](qfec::TableRecoverLaunch& a, hipStream_t s) {
                                  a.out = d_rebuilt;
                                  a.lens = d_shard_lens;
                                  a.symlen = d_symbol_len_out;
                                  QFEC_HIP(qfec::launch_recover_gather_var(a, s));
                                  return FEC_OK;
                                });
  });
}

QFEC_EXPORT int fec_encode_gather_var_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                                             const uint32_t* d_packet_lens, uint64_t G, uint32_t k, uint32_t r,
                                             uint32_t P, uint8_t* d_parity, uint32_t* d_symbol_len_out, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_packet_addrs || !d_packet_lens || !d_parity) {
      set_error("variable-length gather encode: %s is NULL", !ctx              ? "the context"
                                                             : !d_packet_addrs ? "d_packet_addrs"
                                                             : !d_packet_lens  ? "d_packet_lens (the length table)"
                                                                               : "d_parity");
      return FEC_ERR_NULL;
    }
    return table_encode_locked("variable-length gather encode", ctx, G, k, r, P, stream,
                               [&](const void* tables, hipStream_t s) {
                                 // addrs, lens, groups, k, r, P, parity, dests, symlen_out, tables
                                 const qfec::TableEncodeLaunch a{d_packet_addrs, d_packet_lens, G, k, r, P, d_parity, nullptr,
                                                                 d_symbol_len_out, tables};
                                 return table_encode_done(qfec::launch_encode_gather_var(a, s),
                                                          "qfec::launch_encode_gather_var(a, pick_stream(ctx, stream))");
                               });
  });
}

// ---- the recover with a table of destinations (fec_scatter.hip) ----
QFEC_EXPORT int fec_recover_scatter_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                                           const uint32_t* d_shard_lens, const uint64_t* d_dest_addrs, uint64_t G,
                                           uint32_t k, uint32_t r, uint32_t P, uint8_t* d_status,
                                           uint64_t* d_masks_out, uint32_t* d_symbol_len_out, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_shard_addrs || !d_dest_addrs) {
      set_error("scatter recover: %s is NULL", !ctx             ? "the context"
                                               : !d_shard_addrs ? "d_shard_addrs"
                                                                : "d_dest_addrs (the destination table)");
      return FEC_ERR_NULL;
    }
    // behind the record offsets the symbol lengths the kernel cuts its stores at, when there is a
    // length table and the caller asks for none
    const bool own_symlen = d_shard_lens != nullptr && d_symbol_len_out == nullptr;
    return table_recover_locked("scatter recover", ctx, d_shard_addrs, G, k, r, P, d_status, d_masks_out, stream,
                                own_symlen ? 2 : 1,
                                "stream_workspace(ctx, s, (own_symlen ? 2 : 1) * G * sizeof(uint32_t), &ws)",
                                [&](qfec::TableRecoverLaunch& a, hipStream_t s) {
                                  a.lens = d_shard_lens;
                                  a.dests = d_dest_addrs;
                                  if (!own_symlen) a.symlen = d_symbol_len_out;  // else the workspace's
                                  QFEC_HIP(qfec::launch_recover_scatter(a, s));
                                  return FEC_OK;
                                });
  });
}

// ---- the encode with a table of destinations (fec_scatter_encode.hip) ----
QFEC_EXPORT int fec_encode_scatter_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                                          const uint32_t* d_packet_lens, const uint64_t* d_dest_addrs, uint64_t G,
                                          uint32_t k, uint32_t r, uint32_t P, uint32_t* d_symbol_len_out,
                                          void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_packet_addrs || !d_dest_addrs) {
      set_error("scatter encode: %s is NULL", !ctx              ? "the context"
                                              : !d_packet_addrs ? "d_packet_addrs"
                                                                : "d_dest_addrs (the destination table)");
      return FEC_ERR_NULL;
    }
    return table_encode_locked("scatter encode", ctx, G, k, r, P, stream, [&](const void* tables, hipStream_t s) {
      // addrs, lens, groups, k, r, P, parity, dests, symlen_out, tables
      const qfec::TableEncodeLaunch a{d_packet_addrs, d_packet_lens, G, k, r, P, nullptr, d_dest_addrs, d_symbol_len_out,
                                      tables};
      return table_encode_done(qfec::launch_encode_scatter(a, s), "qfec::launch_encode_scatter(a, pick_stream(ctx, stream))");
    });
  });
}

QFEC_EXPORT int fec_decode_prepare(FECEncoderCtx* ctx, uint32_t k, uint32_t r, uint64_t* bytes_out) {
  return api_call(ctx, [&]() -> int {
    if (!ctx) return FEC_ERR_NULL;
    int rc = check_shape(1, k, r, 1, true);
    if (rc != FEC_OK) return rc;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    DecodePlan* plan = nullptr;
    rc = get_decode_plan(ctx, k, r, &plan);
    if (rc != FEC_OK) return rc;
    if (bytes_out) *bytes_out = plan->dense ? plan->layout.total_bytes : 0;  // 0: sparse per-call plans
    if (!plan->dense && ctx->plan_mode == FEC_PLAN_DEVICE) {
      const uint8_t* matrix = nullptr;
      return plan_matrix(plan, &matrix);  // all a device plan keeps between calls
    }
    return FEC_OK;
  });
}

QFEC_EXPORT int fec_fill_random_dev(FECEncoderCtx* ctx, uint8_t* d_dst, uint64_t nbytes, uint64_t seed,
                                    uint64_t byte_offset, void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_dst) return FEC_ERR_NULL;
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    QFEC_HIP(qfec::launch_fill_splitmix(d_dst, nbytes, seed, byte_offset, pick_stream(ctx, stream)));
    return FEC_OK;
  });
}

QFEC_EXPORT int fec_copy_dev(FECEncoderCtx* ctx, const uint8_t* d_src, uint8_t* d_dst, uint64_t nbytes,
                             void* stream) {
  return api_call(ctx, [&]() -> int {
    if (!ctx || !d_src || !d_dst) return FEC_ERR_NULL;
    if (nbytes % 16 || reinterpret_cast<uintptr_t>(d_src) % 16 || reinterpret_cast<uintptr_t>(d_dst) % 16)
    {
      set_error("fec_copy_dev: size and addresses must be multiples of 16");
      return FEC_ERR_RANGE;
    }
    CtxBound bound(ctx);
    if (bound.rc != FEC_OK) return bound.rc;
    QFEC_HIP(qfec::launch_copy_words(d_src, d_dst, nbytes, pick_stream(ctx, stream)));
    return FEC_OK;
  });
}

QFEC_EXPORT int fec_decode_loss_hint(FECEncoderCtx* ctx, double share) {
  if (!ctx) return FEC_ERR_NULL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->decode_need_share = share >= 0.0 && share <= 1.0 ? share : -1.0;
  return FEC_OK;
}

QFEC_EXPORT int fec_decode_plan_mode(FECEncoderCtx* ctx, int mode) {
  return api_call(ctx, [&]() -> int {
    if (!ctx) return FEC_ERR_NULL;
    if (mode != FEC_PLAN_CODEBOOK && mode != FEC_PLAN_DEVICE) {
      set_error("fec_decode_plan_mode: unknown mode %d", mode);
      return FEC_ERR_RANGE;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->plan_mode = mode;
    return FEC_OK;
  });
}

static_assert(FEC_WIDE_ROWS_CAPPED == qfec::kWideRowsCapped && FEC_WIDE_ROWS_ALL == qfec::kWideRowsAll,
              "fec_forms.hpp states the modes for host-only code");
QFEC_EXPORT int fec_wide_rows_mode(FECEncoderCtx* ctx, int mode) {
  return api_call(ctx, [&]() -> int {
    if (!ctx) return FEC_ERR_NULL;
    if (!qfec::wide_rows_mode_known(mode)) {
      set_error("fec_wide_rows_mode: unknown mode %d", mode);
      return FEC_ERR_RANGE;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->wide_rows_mode = mode;
    return FEC_OK;
  });
}

QFEC_EXPORT int fec_synchronize(FECEncoderCtx* ctx) {
  if (!ctx) return FEC_ERR_NULL;
  DeviceGuard dg(ctx->device);
  QFEC_HIP(hipStreamSynchronize(ctx->stream));
  return FEC_OK;
}

// ---------------------------------------------------------------------------------
// Device groups: one host batch sharded over several GPUs.  Groups
// are independent, so shard i of n takes the contiguous range [G*i/n, G*(i+1)/n) and
// runs on its own context (device, streams, staging) from its own host thread; there is
// no exchange between devices.
// ---------------------------------------------------------------------------------
struct FECDeviceGroup {
  std::vector<FECEncoderCtx*> ctxs;
  ~FECDeviceGroup() {
    for (auto* c : ctxs) delete c;
  }
};

namespace {

// Run f(i, g0, n) for every shard, shard 0 on the calling thread; the first failing
// shard's code and message become the caller's.
template <class F>
int for_each_shard(FECDeviceGroup* grp, uint64_t G, F&& f) {
  const uint64_t n = grp->ctxs.size();
  std::vector<int> rc(n, FEC_OK);
  std::vector<std::string> msg(n);
  auto run = [&](uint64_t i) {
    const uint64_t g0 = G * i / n, g1 = G * (i + 1) / n;
    if (g1 > g0) rc[i] = f(i, g0, g1 - g0);
    if (rc[i] != FEC_OK) msg[i] = g_last_error;
  };
  std::vector<std::thread> th;
  for (uint64_t i = 1; i < n; ++i) th.emplace_back(run, i);
  run(0);
  for (auto& t : th) t.join();
  for (uint64_t i = 0; i < n; ++i)
    if (rc[i] != FEC_OK) {
      g_last_error = "shard " + std::to_string(i) + " (device " + std::to_string(grp->ctxs[i]->device) +
                     "): " + msg[i];
      return rc[i];
    }
  return FEC_OK;
}

bool any_device_ptr(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (p && classify_ptr(p) == Mem::kDevice) return true;
  return false;
}

}  // namespace

QFEC_EXPORT FECDeviceGroup* fec_group_new(const int* devices, int ndevices) {
  const int n = fec_hip_device_count();
  if (n <= 0) {
    set_error("fec_group_new: no HIP device available");
    return nullptr;
  }
  std::vector<int> devs;
  if (!devices || ndevices <= 0) {
    for (int d = 0; d < n; ++d) devs.push_back(d);
  } else {
    for (int i = 0; i < ndevices; ++i) {
      if (devices[i] < 0 || devices[i] >= n) {
        set_error("fec_group_new: device %d out of range (%d devices)", devices[i], n);
        return nullptr;
      }
      devs.push_back(devices[i]);
    }
  }
  auto* grp = new FECDeviceGroup();
  for (int d : devs) {
    FECEncoderCtx* c = make_ctx(0.10, 1024, d);
    if (!c) {
      delete grp;
      return nullptr;
    }
    grp->ctxs.push_back(c);
  }
  return grp;
}

QFEC_EXPORT void fec_group_free(FECDeviceGroup* grp) { delete grp; }

QFEC_EXPORT int fec_group_size(const FECDeviceGroup* grp) { return grp ? static_cast<int>(grp->ctxs.size()) : 0; }

QFEC_EXPORT FECEncoderCtx* fec_group_context(FECDeviceGroup* grp, int i) {
  if (!grp || i < 0 || i >= static_cast<int>(grp->ctxs.size())) return nullptr;
  return grp->ctxs[i];
}

QFEC_EXPORT int fec_group_encode_batch_rs(FECDeviceGroup* grp, const uint8_t* data, uint64_t G, uint32_t k,
                                          uint32_t r, uint32_t P, uint8_t* parity_out) {
  if (!grp || !data || !parity_out) return FEC_ERR_NULL;
  int rc = check_shape(G, k, r, P, false);
  if (rc != FEC_OK) return rc;
  if (G == 0) return FEC_OK;
  if (any_device_ptr({data, parity_out})) {
    set_error("fec_group_encode_batch_rs: host buffers only (device buffers belong to one context)");
    return FEC_ERR_RANGE;
  }
  return for_each_shard(grp, G, [&](uint64_t i, uint64_t g0, uint64_t n) {
    return fec_encode_batch_rs(grp->ctxs[i], data + g0 * k * uint64_t(P), nullptr, n, k, r, P,
                               parity_out + g0 * r * uint64_t(P));
  });
}

QFEC_EXPORT int fec_group_decode_batch_rs(FECDeviceGroup* grp, uint8_t* data, const uint8_t* parity,
                                          const uint64_t* masks, uint64_t G, uint32_t k, uint32_t r,
                                          uint32_t P, uint8_t* status_out, uint64_t* unrecoverable_out) {
  if (!grp || !data || !parity || !masks) return FEC_ERR_NULL;
  int rc = check_shape(G, k, r, P, true);
  if (rc != FEC_OK) return rc;
  if (unrecoverable_out) *unrecoverable_out = 0;
  if (G == 0) return FEC_OK;
  if (any_device_ptr({data, parity, masks, status_out})) {
    set_error("fec_group_decode_batch_rs: host buffers only (device buffers belong to one context)");
    return FEC_ERR_RANGE;
  }
  std::vector<uint64_t> bad(grp->ctxs.size(), 0);
  rc = for_each_shard(grp, G, [&](uint64_t i, uint64_t g0, uint64_t n) {
    return fec_decode_batch_rs(grp->ctxs[i], data + g0 * k * uint64_t(P), parity + g0 * r * uint64_t(P),
                               masks + g0, n, k, r, P, status_out ? status_out + g0 : nullptr, &bad[i]);
  });
  if (rc != FEC_OK) return rc;
  if (unrecoverable_out)
    for (uint64_t b : bad) *unrecoverable_out += b;
  return FEC_OK;
}
